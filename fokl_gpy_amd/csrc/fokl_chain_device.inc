// G3 on the device (textually included by fokl_hip.hip): the finishing half of the polar normals and the D-iteration
// recursion of FoKLRoutines.py:1519-1548 in the eigenbasis, for noise tapes recorded by the host's noise thread
// (fokl_hostpool.cpp).  The random STREAM stays on the host -- it is serial by definition -- everything that is only
// arithmetic on it moves to the GPU, which idles 94 % of a fit otherwise:
//
//   tape_gather_kernel   brings a tape into device memory -- read in place from page-locked host memory, no copy calls --
//                        and finishes it on the way: raw accepted polar pairs (x2, x1) -> normals f x2, f x1,
//                        f = sqrt(-2 log r2 / r2), r2 = x1^2 + x2^2 re-formed from the pair (the same two separately
//                        rounded products and one addition the recorder made: fokl_sampler.cpp polar_pairs_raw);
//   gibbs_chain_kernel   (FOKL_DCHAIN_RECURSION=exact) one wavefront per chain.  Lane i + 64 t owns eigen-direction i:
//                        d = 1 / (lamb + 1 / tau2), w = d qty + sigma sqrt(d) v (FR:1521-1528 in the eigenbasis, as
//                        fokl_sampler.cpp chain_step), the three quadratic forms summed in the HOST chain's order (eight
//                        partial sums, element i to partial i mod 8, ascending i, fixed combination tree) so that the
//                        recursion sees the same bits; sigma^2 / tau^2 from the tape's two standard gammas
//                        (FR:1532-1548); the mean of w over the rows the kill tests look at (FR:1671) accumulated on
//                        the fly.  Its results differ from fokl_gibbs_chain only through log(): the device's is within
//                        an ulp of glibc's, which reaches the draws at the 1e-16 level;
//   gibbs_chain_segments_kernel   (the default) the same recursion with its reciprocals folded and its sums in registers
//                        (chain_segment: the one statement of it), as eight verified pieces on eight wavefronts, or
//                        (=serial) as one piece on one.
//
// A small engine around the kernels (fokl_dchain_*): jobs are queued by the driver as soon as a tape is COMMITTED; a
// dispatcher thread sleeps until the recorder has finished that tape, then issues H2D copies, the two kernels and the
// D2H copy of the statistics on one of a few streams (several chains are in flight at once: a chain is ~1 ms of
// dependent latency, a tape arrives every ~0.2 ms).  Waiters sleep on the job's event.  The draws stay in device memory
// until fetched (only the model that is returned needs them) or released.
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <thread>

namespace fokl {

struct ChainArgs {
    const double *lamb, *qty;            // [p1] device
    // the tape as the recorder left it: page-locked host memory read over the bus by tape_gather_kernel, or -- tapes in
    // ordinary memory -- a device staging copy
    const double *src_normals, *src_gam_sig, *src_gam_tau;
    const int32_t *src_lead;
    double *normals;                     // [draws][p1] device, finished
    double *gam_sig, *gam_tau;           // [draws] device
    double *w;                           // [draws][p1] device
    double *stats;                       // [7 + p1] page-locked host memory: flagged, last sigsqd, last tausqd, rows, mean w
                                         // [p1], and -- written last -- the job's ticket: the host's completion flag
    double b, btau, dtd, sigsqd0, tausqd0, ticket;
    double seconds_per_tick;             // of wall_clock64: the kernel times itself (stats[5 + p1], after the ticket's slot;
                                         // stats[6 + p1]: 1.0 when the segmented recursion ran the chain again in one piece)
    int p1, draws, stat_first, finished;
    // the tape as ROWS OF POSITIONS (round 4: fokl_stream_walk): expanded on the device from its own copy of the stream
    const fokl_tape_row *rows;           // [draws] page-locked host memory, or NULL: the arrays above
    const double *x_ring;                // x = 2 d - 1 of every double of the resident segments
    double b_sig, c_sig, b_tau, c_tau;   // Marsaglia-Tsang constants of the two gamma draws (shape - 1/3, 1 / sqrt(9 b))
};

// ---- the device's own copy of the random stream --------------------------------------------------------------------
// The host's bulk threads leave, per segment of 256 MT19937 blocks, the raw block in front of it (fokl_stream_create's
// pre-state ring, page-locked).  One workgroup regenerates a segment from that: the recurrence three phases per block in
// LDS (words 0..226 depend on the block before only, 227..453 on those, 454..623 on those), tempering, numpy's 53-bit
// doubles and x = 2 d - 1 (all exact), written to the segment's slot of a ring in HBM.  The tape rows the host's walker
// records (32 bytes per Gibbs iteration) are then expanded here: which polar attempts were accepted is re-decided from
// x1^2 + x2^2 with the host's two roundings, so flags and positions agree bit for bit.
constexpr int kXRingSegments = 1024;                        // 1024 * 79 872 doubles = 654 MB of HBM

struct SegmentArgs {
    const uint32_t *pre;                                    // a pre-state entry (page-locked host memory)
    double *out;                                            // where the run's doubles go in the ring
};

__device__ __forceinline__ uint32_t mt_twist(uint32_t a, uint32_t b)
{
    const uint32_t y = (a & 0x80000000u) | (b & 0x7fffffffu);
    return (y >> 1) ^ ((0u - (y & 1u)) & 0x9908b0dfu);
}

__device__ __forceinline__ uint32_t mt_temper(uint32_t y)
{
    y ^= (y >> 11);
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= (y >> 18);
    return y;
}

// one workgroup per run of FOKL_PRESTATE_BLOCKS blocks (eight runs make a segment)
__global__ __launch_bounds__(256) void stream_segment_kernel(const SegmentArgs *__restrict__ runs)
{
    const uint32_t *__restrict__ pre = runs[blockIdx.x].pre;
    double *__restrict__ out = runs[blockIdx.x].out;
    __shared__ uint32_t blk[3][640];
    const int t = threadIdx.x;
    for (int i = t; i < 628; i += 256) blk[0][i] = pre[i];
    __syncthreads();
    const int given = (int)blk[0][626], o = (int)blk[0][627] & 1;
    int have = given ? 0 : -1;                              // index (in the run) of the block in blk[cur]
    int cur = 0;
    while (have < FOKL_PRESTATE_BLOCKS) {
        const uint32_t *prev = blk[cur];
        uint32_t *nxt = blk[(cur + 1) % 3];
        if (t < 227) nxt[t] = prev[t + 397] ^ mt_twist(prev[t], prev[t + 1]);
        __syncthreads();
        if (t < 227) nxt[227 + t] = nxt[t] ^ mt_twist(prev[227 + t], prev[228 + t]);
        __syncthreads();
        if (t < 170) {
            const int i = 454 + t;
            nxt[i] = nxt[i - 227] ^ mt_twist(prev[i], i == 623 ? nxt[0] : prev[i + 1]);
        }
        __syncthreads();
        // block `have` is complete and so is the first word behind it: its 312 doubles (double l <-> words o + 2 l,
        // o + 2 l + 1; the last one straddles into the next block when the stream is read from an odd word)
        if (have >= 0) {
            for (int l = t; l < 312; l += 256) {
                const int w0 = o + 2 * l;
                const uint32_t wa = mt_temper(prev[w0]);
                const uint32_t wb = mt_temper(w0 + 1 < 624 ? prev[w0 + 1] : nxt[0]);
                const double d = ((double)(int)(wa >> 5) * 67108864.0 + (double)(int)(wb >> 6)) * (1.0 / 9007199254740992.0);
                out[(size_t)have * 312 + l] = 2.0 * d - 1.0;
            }
        }
        have += 1;
        cur = (cur + 1) % 3;
    }
}

// x of double D of the stream (its segment must be resident)
__device__ __forceinline__ double stream_x(const double *__restrict__ ring, uint64_t D)
{
    const uint64_t seg = D / (uint64_t)FOKL_SEGMENT_DOUBLES;
    return ring[(seg % (uint64_t)kXRingSegments) * (uint64_t)FOKL_SEGMENT_DOUBLES + (D - seg * (uint64_t)FOKL_SEGMENT_DOUBLES)];
}

// the normal a source names: f x1 or f x2 of the accepted attempt at its position (fokl_stream.cpp Walk::value_of)
__device__ __forceinline__ double stream_normal(const double *__restrict__ ring, uint64_t source)
{
    const uint64_t at = source & ~FOKL_SOURCE_X1_HALF;
    const double x1 = stream_x(ring, at), x2 = stream_x(ring, at + 1);
    const double r2 = x1 * x1 + x2 * x2;
    const double f = sqrt(-2.0 * log(r2) / r2);
    return (source & FOKL_SOURCE_X1_HALF) ? f * x1 : f * x2;
}

// blockIdx.y = job of the batch (jobs without rows are left to tape_gather_kernel).  One wavefront per tape row: lane l
// looks at the attempt l places on from where the row's scan stands; the accepted ones are ranked with a ballot and
// written, finished, in the row's order -- after the leading cached normal if there is one, before the half pair that
// closes a row of odd length; lanes 0 and 1 form the two gamma variates.
__global__ __launch_bounds__(256) void tape_expand_kernel(const ChainArgs *__restrict__ jobs)
{
    const ChainArgs a = jobs[blockIdx.y];
    if (!a.rows) return;
    const int lane = threadIdx.x & 63;
    const int waves = (int)(gridDim.x * (blockDim.x >> 6));
    const int p1 = a.p1;
    const double *__restrict__ ring = a.x_ring;
    for (int k = (int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)); k < a.draws; k += waves) {
        const fokl_tape_row row = a.rows[k];
        const int lead = (row.start & FOKL_ROW_LEAD) ? 1 : 0;
        uint64_t D = row.start & ~FOKL_ROW_LEAD;
        double *dst = a.normals + (size_t)k * p1;
        if (lead && lane == 0) dst[0] = stream_normal(ring, row.lead_source | FOKL_SOURCE_X1_HALF);
        const int rest = p1 - lead, pairs = rest >> 1, attempts = (rest + 1) >> 1;
        int have = 0;
        while (have < attempts) {
            const uint64_t at = D + 2 * (uint64_t)lane;
            const double x1 = stream_x(ring, at), x2 = stream_x(ring, at + 1);
            const double r2 = x1 * x1 + x2 * x2;            // the host's flag: two products, one sum, no contraction
            const bool accepted = r2 < 1.0 && r2 != 0.0;
            const unsigned long long mask = __ballot(accepted);
            const int idx = have + __popcll(mask & ((1ull << lane) - 1ull));
            if (accepted && idx < attempts) {
                const double f = sqrt(-2.0 * log(r2) / r2);
                if (idx < pairs) {
                    dst[lead + 2 * idx] = f * x2;
                    dst[lead + 2 * idx + 1] = f * x1;
                } else {
                    dst[p1 - 1] = f * x2;                   // the odd one out: its other half went to the cache
                }
            }
            have += __popcll(mask);
            D += 128;
        }
        if (lane < 2) {
            const uint64_t source = row.gamma[lane];
            const double *from = lane ? a.src_gam_tau : a.src_gam_sig;
            double *to = lane ? a.gam_tau : a.gam_sig;
            if (source == FOKL_GAMMA_FINAL_VALUE) {
                to[k] = from[k];                            // shapes <= 1: the walker stored the variate itself
            } else {
                const double b = lane ? a.b_tau : a.b_sig, c = lane ? a.c_tau : a.c_sig;
                const double X = stream_normal(ring, source);
                double V = 1.0 + c * X;
                V = V * V * V;
                to[k] = b * V;
            }
        }
    }
}


// blockIdx.y = job of the batch.  Brings a tape into device memory and finishes it on the way: thread j of row k takes the
// j-th accepted polar pair (x2, x1) -> (f x2, f x1), f = sqrt(-2 log r2 / r2); thread `pairs` of the row copies the values
// the recorder left final (a leading cached normal, a trailing half pair); the two gamma arrays are copied alongside.
__global__ __launch_bounds__(256) void tape_gather_kernel(const ChainArgs *__restrict__ jobs)
{
    const ChainArgs a = jobs[blockIdx.y];
    if (a.rows) return;                                     // expanded from the device's own stream (tape_expand_kernel)
    const int p1 = a.p1;
    const int half = p1 / 2 + 1;
    const int64_t total = (int64_t)a.draws * half;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int64_t g = first; g < a.draws; g += stride) {
        a.gam_sig[g] = a.src_gam_sig[g];
        a.gam_tau[g] = a.src_gam_tau[g];
    }
    for (int64_t g = first; g < total; g += stride) {
        const int k = (int)(g / half), j = (int)(g - (int64_t)k * half);
        const double *src = a.src_normals + (size_t)k * p1;
        double *dst = a.normals + (size_t)k * p1;
        if (a.finished) {                                   // finished by host threads: a plain copy
            if (2 * j < p1) dst[2 * j] = src[2 * j];
            if (2 * j + 1 < p1) dst[2 * j + 1] = src[2 * j + 1];
            continue;
        }
        const int ld = a.src_lead[k];
        const int pairs = (p1 - ld) / 2;
        if (j < pairs) {
            const double x0 = src[ld + 2 * j], x1 = src[ld + 2 * j + 1];
            const double r2 = x1 * x1 + x0 * x0;           // out[2 i] = x2, out[2 i + 1] = x1: rr = x1^2 + x2^2
            const double f = sqrt(-2.0 * log(r2) / r2);
            dst[ld + 2 * j] = f * x0;
            dst[ld + 2 * j + 1] = f * x1;
        } else if (j == pairs) {
            if (ld) dst[0] = src[0];
            if ((p1 - ld) & 1) dst[p1 - 1] = src[p1 - 1];
        }
    }
}

// Loads / stores through address space 1: from a generic pointer hipcc emits flat_load / flat_store, which count on
// lgkmcnt as well -- every wait for an LDS read then waits out the global loads just issued (the prefetch ring below would
// be worth nothing: one memory latency per Gibbs iteration, 0.7 us).
__device__ __forceinline__ double gload(const double *p) { return *(global_cd_ptr)(p); }
__device__ __forceinline__ void gstore(double *p, double v) { *(global_d_ptr)(p) = v; }

// Lane i takes the value of lane i + N of its row of 16 (DPP row_shl: no LDS crossbar, a few cycles).
template <int N>
__device__ inline double row_down(double x)
{
    const int lo = __double2loint(x), hi = __double2hiint(x);
    const int lo2 = __builtin_amdgcn_update_dpp(lo, lo, 0x100 + N, 0xf, 0xf, false);
    const int hi2 = __builtin_amdgcn_update_dpp(hi, hi, 0x100 + N, 0xf, 0xf, false);
    return __hiloint2double(hi2, lo2);
}

// The value of lane `lane` (a constant) in every lane.
__device__ inline double from_lane(double x, int lane)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(x), lane);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(x), lane);
    return __hiloint2double(hi, lo);
}

// 1 / sqrt(x) and 1 / x for x > 0 from the hardware seeds (v_rsq_f64 / v_rcp_f64: ~2^-27 relative) and two Newton steps each,
// spelled with explicit fused operations: within an ulp or two of the correctly rounded results, in a third of the
// instructions the IEEE division / square root sequences take -- which stand on the recursion's critical path.
__device__ __forceinline__ double rsq_newton(double x)
{
    double y = __builtin_amdgcn_rsq(x);
    double e = __builtin_fma(-x * y, y, 1.0);
    y = __builtin_fma(0.5 * y, e, y);
    e = __builtin_fma(-x * y, y, 1.0);
    return __builtin_fma(0.5 * y, e, y);
}

// One Newton step from the hardware seeds (2^-27 relative -> ~2^-53 before the step's own roundings): what stands on the
// recursion's critical path (FAST).  The draws are held to 1e-9 of the reference's; these are good to an ulp or two.
__device__ __forceinline__ double rsq_newton1(double x)
{
    const double y = __builtin_amdgcn_rsq(x);
    const double e = __builtin_fma(-x * y, y, 1.0);
    return __builtin_fma(0.5 * y, e, y);
}

__device__ __forceinline__ double rcp_newton1(double x)
{
    const double y = __builtin_amdgcn_rcp(x);
    const double e = __builtin_fma(-x, y, 1.0);
    return __builtin_fma(y, e, y);
}

__device__ __forceinline__ double rcp_newton(double x)
{
    double y = __builtin_amdgcn_rcp(x);
    double e = __builtin_fma(-x, y, 1.0);
    y = __builtin_fma(y, e, y);
    e = __builtin_fma(-x, y, 1.0);
    return __builtin_fma(y, e, y);
}

// Sum over the 64 lanes, in every lane: four DPP steps inside each row of 16 (lane 0 of a row ends up with the row's sum),
// then the four row sums through scalar registers.  No LDS, no barrier.
__device__ __forceinline__ double wave_total(double x)
{
    x += row_down<8>(x);
    x += row_down<4>(x);
    x += row_down<2>(x);
    x += row_down<1>(x);
    return (from_lane(x, 0) + from_lane(x, 16)) + (from_lane(x, 32) + from_lane(x, 48));
}

// The ticket is the completion flag the host polls (plain loads from its own page-locked memory -- no runtime call); every
// kernel that completes this way ends here (spectral_vectors_kernel too).  All wavefronts of the workgroup have stored into
// host memory: each one makes its own stores visible system-wide FIRST, the barrier then tells thread 0 that every fence is
// behind, and only then is the ticket stored.  (Barrier first, fences second let thread 0 pass its own fence and publish the
// ticket while another wavefront's stores were still on their way: the barrier does not wait for outstanding stores.)
__device__ __forceinline__ void publish_ticket(double *word, double ticket)
{
    __threadfence_system();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // (the fence's own wait, spelled out: the compiler may not drop it)
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(word, ticket, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// FOKL_DCHAIN_RECURSION=exact.  blockIdx.x = job of the batch (all of one size class T = elements per lane); one wavefront
// per chain.  The host chain's operations in the host chain's order (fokl_sampler.cpp chain_step) -- on finished normals the
// draws are the host's bit for bit; nine divisions / square roots stand in a row on the recursion's critical path, ~1 us per
// Gibbs iteration.
template <int T>
__global__ __launch_bounds__(64) void gibbs_chain_kernel(const ChainArgs *__restrict__ jobs)
{
    // rows of normals (and the two gammas) are fetched U iterations ahead into a ring of registers: a row's load is a
    // trip to L2 / HBM (~1 us), an iteration of the recursion a fraction of that -- fetched one iteration ahead, as the
    // first version did, every iteration waited out a memory latency
    constexpr int U = T <= 2 ? 8 : (T <= 4 ? 4 : 2);
    __shared__ double red[2][3][64 * T];                    // double-buffered: one barrier per iteration
    // the two gammas of GCH iterations at a time in LDS (the compiler sinks a register ring of wave-uniform loads back to
    // their use: one memory latency per iteration again).  Small on purpose: a chain shares its CU with workgroups of the
    // fit's Gram launches, which take up to 136 of the 160 KB of LDS -- with 16 KB of gammas here such a workgroup did not
    // fit next to a chain, ran after the others, and the launch took up to twice as long (fp64-MFMA-bound Gram launches
    // in situ: 0.70 of the peak without chains on the device, 0.55 with)
    constexpr int GCH = 128;
    __shared__ double gam[2][GCH];
    const ChainArgs a = jobs[blockIdx.x];
    const long long t_begin = wall_clock64();
    const int lane = threadIdx.x, p1 = a.p1, draws = a.draws;
    double lam[T], qt[T], sum_w[T];
    double vbuf[U][T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
        const int i = lane + 64 * t;
        lam[t] = i < p1 ? gload(a.lamb + i) : 1.0;
        qt[t] = i < p1 ? gload(a.qty + i) : 0.0;
        sum_w[t] = 0.0;
    }
    // Loads are unconditional on clamped indices (a select on a loaded value makes the compiler wait for the load where
    // the select stands; lanes beyond p1 and rows beyond the last compute values nobody stores or sums).
    int col[T];
#pragma unroll
    for (int t = 0; t < T; ++t) col[t] = min(lane + 64 * t, p1 - 1);
    const int last = max(draws - 1, 0);
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int ku = min(u, last);
#pragma unroll
        for (int t = 0; t < T; ++t) vbuf[u][t] = gload(a.normals + (size_t)ku * p1 + col[t]);
    }
    double sigsqd = a.sigsqd0, tausqd = a.tausqd0;
    int flagged = 0;
    const int s = lane >> 3, l = lane & 7;                  // lanes 0..23: partial l of sum s
    for (int k0 = 0; k0 < draws; k0 += U) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int k = k0 + u;
            if (k >= draws) break;                          // uniform
            if ((k & (GCH - 1)) == 0) {                     // uniform: the next GCH iterations' gammas
                __syncthreads();
                for (int j = lane; j < GCH; j += 64) {
                    const int kj = min(k + j, last);
                    gam[0][j] = gload(a.gam_sig + kj);
                    gam[1][j] = gload(a.gam_tau + kj);
                }
                __syncthreads();
            }
            const double gs = gam[0][k & (GCH - 1)], gt = gam[1][k & (GCH - 1)];
            double (*buf)[64 * T] = red[k & 1];
            const double *mine = buf[s < 3 ? s : 0];
            const double inv_tau = 1.0 / tausqd;
            const double sig = sqrt(sigsqd);
#pragma unroll
            for (int t = 0; t < T; ++t) {
                const int i = lane + 64 * t;
                const double d = 1.0 / (lam[t] + inv_tau);
                const double root = sqrt(d);
                const double wi = d * qt[t] + sig * (root * vbuf[u][t]);
                const double ww = wi * wi;
                if (i < p1) {
                    gstore(a.w + (size_t)k * p1 + i, wi);
                    buf[0][i] = lam[t] * ww;
                    buf[1][i] = wi * qt[t];
                    buf[2][i] = ww;
                    if (k >= a.stat_first) sum_w[t] += wi;
                }
            }
            // this slot of the ring is free: row k + U goes into it (consumed U iterations from now)
            {
                const int kn = min(k + U, last);
#pragma unroll
                for (int t = 0; t < T; ++t) vbuf[u][t] = gload(a.normals + (size_t)kn * p1 + col[t]);
            }
            __syncthreads();
            // the host chain's order (fokl_sampler.cpp chain_vector_portable): partial l takes the elements i = l,
            // l + 8, ... in ascending order; all reads issued before the dependent additions (compile-time trip count)
            // (elements beyond p1 enter as + 0.0, which leaves a partial sum as it is; branch-free)
            double x[8 * T];
#pragma unroll
            for (int j = 0; j < 8 * T; ++j) x[j] = mine[min(l + 8 * j, 64 * T - 1)];
            double acc = 0.0;
#pragma unroll
            for (int j = 0; j < 8 * T; ++j) acc += (l + 8 * j < p1) ? x[j] : 0.0;
            // ((p0 + p4) + (p2 + p6)) + ((p1 + p5) + (p3 + p7)) inside each group of eight lanes
            acc += row_down<4>(acc);
            acc += row_down<2>(acc);
            acc += row_down<1>(acc);
            const double q_lam = from_lane(acc, 0), q_ty = from_lane(acc, 8), q_ww = from_lane(acc, 16);
            const double bstar = a.b + 0.5 * (q_lam - 2.0 * q_ty + a.dtd + q_ww / tausqd);
            if (bstar < 0.0) {
                flagged = 1;                                // the tape holds a gamma the reference would not have drawn
                sigsqd = __builtin_nan("");
            } else {
                sigsqd = 1.0 / ((1.0 / bstar) * gs);
            }
            const double btau_star = (1.0 / (2.0 * sigsqd)) * q_ww + a.btau;
            tausqd = 1.0 / ((1.0 / btau_star) * gt);
        }
    }
    const int rows = draws > a.stat_first ? draws - a.stat_first : 0;
#pragma unroll
    for (int t = 0; t < T; ++t) {
        const int i = lane + 64 * t;
        if (i < p1) gstore(a.stats + 4 + i, rows > 0 ? sum_w[t] / (double)rows : 0.0);
    }
    if (lane == 0) {
        gstore(a.stats + 0, (double)flagged);
        gstore(a.stats + 1, sigsqd);
        gstore(a.stats + 2, tausqd);
        gstore(a.stats + 3, (double)rows);
        gstore(a.stats + 5 + p1, (double)(wall_clock64() - t_begin) * a.seconds_per_tick);   // the chain's own duration
        gstore(a.stats + 6 + p1, 0.0);                      // (no cut to fail: a recycled slot never shows an old 1)
    }
    publish_ticket(a.stats + 4 + p1, a.ticket);
}

// ---- the FAST recursion (FOKL_DCHAIN_RECURSION = fast, the default, or serial) -------------------------------------------
// The same recursion as gibbs_chain_kernel's with the reciprocals folded --
//     sigma^2' = bstar / g_s                      for 1 / ((1 / bstar) g_s)
//     1/tau^2' = 2 g_t bstar / (C g_s + 2 btau bstar)   for 1 / (1 / ((1 / btau*) g_t)),  btau* = C / (2 sigma^2') + btau
//     C / tau^2 = C * (1/tau^2)
// -- which leaves three long operations on the critical path (d = 1 / (lamb + 1/tau^2), sqrt(d), the quotient of
// 1/tau^2').  Round 5: those three are Newton-refined hardware seeds (s = rsq(lamb + 1/tau^2), sqrt(d) = s, d = s s;
// sigma = sqrt(bstar) rsq(g_s) with rsq(g_s) formed when the gammas are staged; the quotient as a product with rcp), and
// the three sums of an iteration are formed in registers (per-lane partial over its T elements, DPP steps inside the rows
// of 16, the four row sums through scalar registers) instead of in the host chain's order through LDS and a barrier: 0.53
// -> 0.3x us per iteration at up to 64 columns.  Every such step differs from the host's by a rounding or two; the chain
// does not amplify that (draws agree with the host chain to ~1e-15 of the column scale, bounded by 1e-13 in
// tests/test_chain_device.py).
// Round 6: two of the three sums leave the critical path.  With A = sqrt(d) qty, B = sigma v (w = sqrt(d) (A + B)):
//     (lamb + 1/tau^2) w^2 - 2 w qty = (A + B)^2 - 2 A (A + B) = B^2 - A^2,
// so   bstar = b + (dtd - sum_j d_j qty_j^2 + sigma^2 sum_j v_j^2) / 2:
// the sum of a row's squared normals does not depend on the recursion at all (formed beside it, on the same wavefront, from
// the row already in registers), sum_j d_j qty_j^2 needs d alone, and sum_j w_j^2 (for 1/tau^2') is the only sum behind w.
// The seeds take ONE Newton step (rsq_newton1 / rcp_newton1), sigma' = bstar rsq(bstar) rsq(g_s).  Dependent instructions
// per iteration ~48 -> ~33: 1.05 -> 0.7x ms per 2000 iterations at up to 64 columns.
//
// IN SEGMENTS (round 6).  The D-iteration loop is a chain only through two scalars, sigma^2 and 1/tau^2, and it forgets them
// fast: bstar carries the old sigma^2 with the weight sum v^2 / 2 against a gamma variate of shape ~ n / 2 (a factor ~ p1 / n per iteration), and
// 1/tau^2 enters through d_j = 1 / (lamb_j + 1/tau^2), next to nothing where lamb_j is large.  So the 2000 iterations are cut
// into kChainSegments pieces, one wavefront each, side by side in one workgroup: piece s starts kChainWarm iterations EARLY
// from the chain's initial state, throws those iterations away, and must arrive at its first real iteration with the state the
// piece before it ENDS on -- which is checked (both scalars to 1e-14 relative) once all pieces have run.  A chain whose state
// is not forgotten that fast (a prior precision comparable to its small eigenvalues) fails the check and is run again by one
// wavefront from start to end, as before (stats[6 + p1] says so, and the engine counts such chains: they are paid for
// twice).  A cut that passes is exact to the check's tolerance, not to the bit: the draws of an accepted cut agree with the
// one-piece recursion to 1e-14 times O(1) (contraction, no growth), those of a chain that was run again are the one-piece
// recursion's bits.  2000 iterations become 314 dependent ones: 0.9 ms -> 0.15 ms per chain, and the chain of a sub-stage's
// model is what its statistics -- hence its kill tests -- wait for.
constexpr int kChainSegments = FOKL_CHAIN_SEGMENTS;         // (fokl_hip_internal.h: the host chain cuts the same way)
constexpr int kChainWarm = FOKL_CHAIN_WARM;
constexpr int kChainGammas = 32;                            // gammas staged per wavefront at a time (wave-private LDS)

template <int T>
struct ChainLane {
    double lam[T], qt[T], qt2[T];
    int col[T];
};

// The one statement of the fast iteration: a piece of the default kernel, its one-wavefront fallback and the whole chain of
// FOKL_DCHAIN_RECURSION=serial all run it, which is what "the fallback equals the serial mode bit for bit" rests on.
// Iterations [k_begin, k_end) on one wavefront; rows before k_write are warm-up (nothing stored, nothing summed); the state
// in front of iteration k_write is left in at_write[0..1].  gam: this wavefront's [3][kChainGammas] of LDS.
template <int T>
__device__ __forceinline__ void chain_segment(const ChainArgs &a, const ChainLane<T> &c, int lane, double *gam, int k_begin,
                                              int k_write, int k_end, double &sigsqd, double &inv_tau, double &sig,
                                              double (&sum_w)[T], int &flagged, double (&at_write)[2])
{
    // rows of normals are fetched U iterations ahead into a ring of registers (see gibbs_chain_kernel)
    constexpr int U = T <= 2 ? 8 : (T <= 4 ? 4 : 2);
    constexpr int G = kChainGammas;
    const int p1 = a.p1, last = max(a.draws - 1, 0);
    double vbuf[U][T];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int ku = min(k_begin + u, last);
#pragma unroll
        for (int t = 0; t < T; ++t) vbuf[u][t] = gload(a.normals + (size_t)ku * p1 + c.col[t]);
    }
    for (int k0 = k_begin; k0 < k_end; k0 += U) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int k = k0 + u;
            if (k >= k_end) break;                          // uniform
            const int g = (k - k_begin) & (G - 1);
            if (g == 0) {                                   // uniform: the next G iterations' gammas, for this wavefront alone
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                if (lane < G) {
                    const int kj = min(k + lane, last);
                    const double g_s = gload(a.gam_sig + kj);
                    gam[lane] = g_s;
                    gam[G + lane] = gload(a.gam_tau + kj);
                    gam[2 * G + lane] = rsq_newton(g_s);
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            }
            const double gs = gam[g], gt = gam[G + g], r_gs = gam[2 * G + g];
            if (k == k_write) {
                at_write[0] = sigsqd;
                at_write[1] = inv_tau;
            }
            const bool real = k >= k_write;
            double part_f = 0.0, part_vv = 0.0, part_ww = 0.0;              // this lane's share of the three sums
#pragma unroll
            for (int t = 0; t < T; ++t) {
                const int i = lane + 64 * t;
                const double v = vbuf[u][t];
                const double bv = sig * v;                                  // (off the critical path: sigma is known early)
                const double root = rsq_newton1(c.lam[t] + inv_tau);
                const double d = root * root;
                const double z = __builtin_fma(root, c.qt[t], bv);
                const double wi = root * z;
                if (i < p1) {
                    if (real) gstore(a.w + (size_t)k * p1 + i, wi);
                    part_f = __builtin_fma(c.qt2[t], d, part_f);
                    part_vv = __builtin_fma(v, v, part_vv);
                    part_ww = __builtin_fma(wi, wi, part_ww);
                    if (real && k >= a.stat_first) sum_w[t] += wi;
                }
            }
            // this slot of the ring is free: row k + U goes into it (consumed U iterations from now)
            {
                const int kn = min(k + U, last);
#pragma unroll
                for (int t = 0; t < T; ++t) vbuf[u][t] = gload(a.normals + (size_t)kn * p1 + c.col[t]);
            }
            const double q_vv = wave_total(part_vv);                        // (independent of the recursion)
            const double q_f = wave_total(part_f), q_ww = wave_total(part_ww);
            const double bstar = a.b + 0.5 * ((a.dtd - q_f) + sigsqd * q_vv);
            if (bstar < 0.0) {
                if (real) flagged = 1;                      // the tape holds a gamma the reference would not have drawn
                sigsqd = __builtin_nan("");
                inv_tau = __builtin_nan("");
                sig = __builtin_nan("");
            } else {
                const double two_b = 2.0 * bstar;
                inv_tau = (gt * two_b) * rcp_newton1(q_ww * gs + a.btau * two_b);   // the next iteration's critical path
                // (bstar == 0: sigma = 0 without 0 * inf; bstar NaN -- the rows behind a flagged one -- stays NaN, as
                // the host chain's last sigma^2 does)
                sig = bstar > 0.0 ? (bstar * rsq_newton1(bstar)) * r_gs : bstar;
                sigsqd = sig * sig;
            }
        }
    }
}

// blockIdx.x = job of the batch; S wavefronts per chain: kChainSegments pieces (see above), or -- S = 1,
// FOKL_DCHAIN_RECURSION=serial -- the whole chain as the one piece of one wavefront: no cut to check, bad_cut stays 0
template <int T, int S = kChainSegments>
__global__ __launch_bounds__(64 * S) void gibbs_chain_segments_kernel(const ChainArgs *__restrict__ jobs)
{
    __shared__ double gam[S][3 * kChainGammas];
    __shared__ double begin_state[S][2], end_state[S][2];
    __shared__ double mean_acc[64 * T];
    __shared__ int any_flag, bad_cut;
    const ChainArgs a = jobs[blockIdx.x];
    const long long t_begin = wall_clock64();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, p1 = a.p1, draws = a.draws;
    ChainLane<T> c;
    double sum_w[T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
        const int i = lane + 64 * t;
        c.lam[t] = i < p1 ? gload(a.lamb + i) : 1.0;
        c.qt[t] = i < p1 ? gload(a.qty + i) : 0.0;
        c.qt2[t] = c.qt[t] * c.qt[t];
        c.col[t] = min(i, p1 - 1);                          // (loads on clamped indices: see gibbs_chain_kernel)
        sum_w[t] = 0.0;
    }
    if (threadIdx.x == 0) {
        any_flag = 0;
        bad_cut = 0;
    }
    for (int i = threadIdx.x; i < 64 * T; i += 64 * S) mean_acc[i] = 0.0;
    // pieces of `piece` iterations; a chain too short to be worth cutting runs as one piece on wavefront 0
    const int pieces = draws >= 4 * kChainWarm ? S : 1;
    const int piece = (draws + pieces - 1) / pieces;
    const int k_write = min(wave * piece, draws), k_end = wave < pieces ? min(k_write + piece, draws) : k_write;
    const int k_begin = max(k_write - kChainWarm, 0);
    double sigsqd = a.sigsqd0, inv_tau = 1.0 / a.tausqd0, sig = sqrt(a.sigsqd0);
    int flagged = 0;
    double at_write[2] = {sigsqd, inv_tau};
    if (k_end > k_write) chain_segment<T>(a, c, lane, gam[wave], k_begin, k_write, k_end, sigsqd, inv_tau, sig, sum_w, flagged, at_write);
    if (lane == 0) {
        begin_state[wave][0] = at_write[0];
        begin_state[wave][1] = at_write[1];
        end_state[wave][0] = sigsqd;
        end_state[wave][1] = inv_tau;
    }
    __syncthreads();
    // every piece but the first must have begun where the piece before it ended
    if (threadIdx.x == 0) {
        int bad = 0;
        for (int w2 = 1; w2 < pieces; ++w2) {
            if (min(w2 * piece, draws) >= draws) break;     // (an empty piece)
            for (int j = 0; j < 2; ++j) {
                const double want = end_state[w2 - 1][j], have = begin_state[w2][j];
                if (!(fabs(have - want) <= 1e-14 * fabs(want))) bad = 1;
            }
        }
        bad_cut = bad;
    }
    __syncthreads();
    if (S > 1 && bad_cut) {
        // not forgotten within the warm-up: the whole chain on one wavefront, from the initial state (rows rewritten)
        if (wave == 0) {
#pragma unroll
            for (int t = 0; t < T; ++t) sum_w[t] = 0.0;
            sigsqd = a.sigsqd0;
            inv_tau = 1.0 / a.tausqd0;
            sig = sqrt(a.sigsqd0);
            flagged = 0;
            chain_segment<T>(a, c, lane, gam[0], 0, 0, draws, sigsqd, inv_tau, sig, sum_w, flagged, at_write);
            if (lane == 0) {
                end_state[S - 1][0] = sigsqd;
                end_state[S - 1][1] = inv_tau;
            }
        } else {
#pragma unroll
            for (int t = 0; t < T; ++t) sum_w[t] = 0.0;
            flagged = 0;
        }
    } else if (lane == 0 && wave == pieces - 1 && pieces < S) {
        end_state[S - 1][0] = sigsqd;                       // (one piece: its end is the chain's)
        end_state[S - 1][1] = inv_tau;
    }
    if (flagged && lane == 0) atomicOr(&any_flag, 1);
    // the mean of w over the rows the kill tests look at: the pieces' sums in piece order (the same bits every time; a sum
    // starts at + 0.0 and never becomes - 0.0, so 0.0 + sum is the sum itself: one piece's mean is its own sum's quotient)
    for (int w2 = 0; w2 < S; ++w2) {
        __syncthreads();
        if (wave == w2) {
#pragma unroll
            for (int t = 0; t < T; ++t) mean_acc[lane + 64 * t] += sum_w[t];
        }
    }
    __syncthreads();
    const int rows = draws > a.stat_first ? draws - a.stat_first : 0;
    for (int i = threadIdx.x; i < p1; i += 64 * S) gstore(a.stats + 4 + i, rows > 0 ? mean_acc[i] / (double)rows : 0.0);
    if (threadIdx.x == 0) {
        // (the last piece that ran is the one that holds the chain's end; empty trailing pieces copy nothing)
        int last_piece = pieces - 1;
        while (last_piece > 0 && min(last_piece * piece, draws) >= draws) --last_piece;
        const double *fin = bad_cut || pieces < S ? end_state[S - 1] : end_state[last_piece];
        gstore(a.stats + 0, (double)any_flag);
        gstore(a.stats + 1, fin[0]);
        gstore(a.stats + 2, 1.0 / fin[1]);
        gstore(a.stats + 3, (double)rows);
        gstore(a.stats + 5 + p1, (double)(wall_clock64() - t_begin) * a.seconds_per_tick);
        gstore(a.stats + 6 + p1, (double)bad_cut);          // this chain ran as one piece after all (DeviceChainJob.bad_cut)
    }
    publish_ticket(a.stats + 4 + p1, a.ticket);             // (means of the columns from 64 on and rows of w: all S wavefronts)
}


}  // namespace fokl

namespace {

constexpr int kChainMaxT = 12;                              // elements per lane: models of up to 768 columns
constexpr int kChainStreams = 4;                            // at most; FOKL_DCHAIN_STREAMS (default 4) are used
constexpr int kChainBatchMax = 32;
constexpr int kChainBatches = 12;                           // batch records in rotation

struct ChainSlot {
    // device buffers (grow only)
    double *d_normals = nullptr, *d_w = nullptr, *d_small = nullptr;    // small: gam_sig | gam_tau | stats
    int32_t *d_lead = nullptr;
    double *h_stats = nullptr;                                          // pinned
    size_t cap_rows_p1 = 0, cap_small = 0, cap_draws = 0, cap_stats = 0;
    bool busy = false;
    int64_t ticket = 0;                                                 // of the job that holds the slot (or held it last)
};

// What one launch works through: the jobs' argument records and model vectors in page-locked memory, which the kernels
// read in place (no copy call, no event: a batch is complete when each of its jobs has stored its ticket).
struct ChainBatch {
    char *h_stage = nullptr;                                            // [kChainBatchMax ChainArgs | models]
    size_t cap = 0;
    fokl::SegmentArgs *h_runs = nullptr;                                // pre-state runs this batch's launch regenerates
    int runs_cap = 0;
    struct Flag {
        const double *word;                                             // a job's completion word ...
        int64_t ticket;                                                 // ... the value that says it has run ...
        int slot;                                                       // ... and the slot it lives in
    };
    std::vector<Flag> flags;
    hipStream_t stream = nullptr;
    // segments of the stream's ring this batch's expansion reads (rows mode), until every job of it has run
    int64_t seg_lo = 0, seg_hi = -1;
};

struct ChainJob {
    int64_t ticket = 0;
    int slot = -1;
    int p1 = 0, draws = 0, stat_first = 0, finished = 0;
    double b = 0, btau = 0, dtd = 0, sigsqd0 = 0, tausqd0 = 0;
    std::vector<double> model;                                          // lamb | qty (copied at submit)
    const double *normals = nullptr, *gam_sig = nullptr, *gam_tau = nullptr;
    const int32_t *lead = nullptr, *progress = nullptr, *block_done = nullptr;
    int block = 0;
    // rows mode (fokl_dchain_submit_rows)
    const fokl_tape_row *rows = nullptr;
    const uint64_t *span = nullptr;                                     // [first position held, position behind the tape]
    double astar = 0, atau_star = 0;
    int state = 0;                                                      // 0 queued, 1 issued, 2 failed
    hipStream_t stream = nullptr;                                       // where it was issued
    int status = FOKL_OK;
    std::string error;
    int64_t t_submit = 0;
    std::atomic<bool> counted{false};                                   // its fallback indicator has been added to `recuts`
};

}  // namespace

struct fokl_dchain {
    int device = 0;
    hipStream_t streams[kChainStreams] = {};
    int next_stream = 0, next_batch = 0, n_streams = 4;
    std::vector<ChainSlot> slots;
    ChainBatch batches[kChainBatches];
    std::mutex m;
    std::condition_variable cv_queue, cv_state;
    std::deque<ChainJob *> queue;
    std::map<int64_t, ChainJob *> jobs;                                 // every job not released yet
    int64_t next_ticket = 1;
    bool stop = false;
    int flush = 0;                                                      // somebody waits: issue what is there at once
    bool fast = true;                                                   // FOKL_DCHAIN_RECURSION = fast (default) | exact
    bool segments = true;                                               // ... | serial: the fast recursion on one wavefront
    double seconds_per_tick = 1e-8;                                     // wall_clock64 (hipDeviceAttributeWallClockRate)
    int batch_target = 16;                                              // FOKL_DCHAIN_BATCH
    int64_t batch_delay_ns = 1000000;                                   // FOKL_DCHAIN_DELAY_US
    // the device's own copy of the random stream (rows mode)
    uint32_t *pre_ring = nullptr;                                       // page-locked: the host's bulk threads write it
    int pre_entries = 0;
    double *x_ring = nullptr;                                           // [kXRingSegments * FOKL_SEGMENT_DOUBLES] device
    std::vector<int64_t> resident;                                      // segment in each ring slot, -1: none
    const fokl_stream *bound = nullptr;                                 // whose pre-states the ring holds right now
    hipEvent_t seg_events[kChainStreams] = {};                          // behind the last segment launch of each stream
    bool seg_recorded[kChainStreams] = {};
    std::atomic<int64_t> segments_made{0}, rows_jobs{0};
    std::thread dispatcher;
    std::atomic<int64_t> busy_ns{0}, issued{0}, launches{0}, staged{0};
    std::atomic<int64_t> recuts{0};                                     // chains that failed their cut and ran again in one piece
    int64_t ph[6] = {0, 0, 0, 0, 0, 0};   // development: where the dispatcher's time goes (FOKL_DCHAIN_TRACE)
    std::string err;
};

namespace {

inline int64_t dchain_now_ns()
{
    return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch())
        .count();
}

int dchain_fail(fokl_dchain *e, int code, const std::string &msg)
{
    if (e) e->err = msg;
    fokl_set_global_error(msg);
    if (std::getenv("FOKL_DCHAIN_TRACE")) std::fprintf(stderr, "fokl_dchain: error %d: %s\n", code, msg.c_str());
    return code;
}

#define DCHAIN_TRY(e, call)                                                                                    \
    do {                                                                                                       \
        hipError_t e__ = (call);                                                                               \
        if (e__ != hipSuccess)                                                                                 \
            return dchain_fail(e, FOKL_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e__));           \
    } while (0)

int ensure_slot(fokl_dchain *e, ChainSlot &s, int p1, int draws)
{
    const size_t rows_p1 = (size_t)draws * p1;
    if (rows_p1 > s.cap_rows_p1) {
        if (s.d_normals) DCHAIN_TRY(e, hipFree(s.d_normals));
        if (s.d_w) DCHAIN_TRY(e, hipFree(s.d_w));
        s.d_normals = s.d_w = nullptr;
        s.cap_rows_p1 = 0;
        const size_t cap = rows_p1 + rows_p1 / 4 + 64;
        DCHAIN_TRY(e, hipMalloc((void **)&s.d_normals, cap * sizeof(double)));
        DCHAIN_TRY(e, hipMalloc((void **)&s.d_w, cap * sizeof(double)));
        s.cap_rows_p1 = cap;
    }
    const size_t small = 4 * (size_t)draws;                 // gam_sig | gam_tau | staging of the two (tapes not page-locked)
    if (small > s.cap_small) {
        if (s.d_small) DCHAIN_TRY(e, hipFree(s.d_small));
        s.d_small = nullptr;
        s.cap_small = 0;
        const size_t cap = small + small / 4 + 64;
        DCHAIN_TRY(e, hipMalloc((void **)&s.d_small, cap * sizeof(double)));
        s.cap_small = cap;
    }
    if ((size_t)draws > s.cap_draws) {
        if (s.d_lead) DCHAIN_TRY(e, hipFree(s.d_lead));
        s.d_lead = nullptr;
        s.cap_draws = 0;
        DCHAIN_TRY(e, hipMalloc((void **)&s.d_lead, ((size_t)draws + 64) * sizeof(int32_t)));
        s.cap_draws = (size_t)draws + 64;
    }
    return FOKL_OK;
}

// the slot's statistics area (page-locked: the recursion kernel writes it, the host polls its last word).  Allocated ONCE
// per slot, for the largest model the engine takes: batch records and the caller remember its address.
int ensure_stats(fokl_dchain *e, ChainSlot &s, int p1)
{
    (void)p1;
    if (!s.h_stats) {
        const size_t cap = (size_t)6 + 64 * kChainMaxT + 64;
        DCHAIN_TRY(e, hipHostMalloc((void **)&s.h_stats, cap * sizeof(double)));
        s.cap_stats = cap;
    }
    return FOKL_OK;
}

// Page-locked blocks handed out by fokl_host_alloc: the device reads a tape that lies in one of them in place.  (Asking the
// runtime about a pointer -- hipPointerGetAttributes -- costs the dispatcher more than the copies it would save.)
std::mutex g_pinned_mutex;
std::map<uintptr_t, size_t> g_pinned_blocks;

bool device_can_read(const void *ptr, size_t bytes)
{
    std::lock_guard<std::mutex> lock(g_pinned_mutex);
    const uintptr_t at = reinterpret_cast<uintptr_t>(ptr);
    auto it = g_pinned_blocks.upper_bound(at);
    if (it == g_pinned_blocks.begin()) return false;
    --it;
    return at >= it->first && at + bytes <= it->first + it->second;
}

// FOKL_DCHAIN_RECURSION when the engine was created: the fast recursion in segments (default), the same statement as one
// piece on one wavefront from start to end (serial: segments == false), or the host chain's own operations (exact)
template <int T>
void launch_chain(const fokl::ChainArgs *d_jobs, int count, hipStream_t stream, bool fast, bool segments)
{
    if (fast && segments)
        hipLaunchKernelGGL((fokl::gibbs_chain_segments_kernel<T>), dim3((unsigned)count), dim3(64 * fokl::kChainSegments), 0,
                           stream, d_jobs);
    else if (fast)
        hipLaunchKernelGGL((fokl::gibbs_chain_segments_kernel<T, 1>), dim3((unsigned)count), dim3(64), 0, stream, d_jobs);
    else
        hipLaunchKernelGGL((fokl::gibbs_chain_kernel<T>), dim3((unsigned)count), dim3(64), 0, stream, d_jobs);
}

inline int chain_class(int p1)
{
    const int T = (p1 + 63) / 64;
    return T <= 1 ? 1 : T <= 2 ? 2 : T <= 3 ? 3 : T <= 4 ? 4 : T <= 6 ? 6 : T <= 8 ? 8 : kChainMaxT;
}

// Segments [first / S, last / S] of the bound stream are wanted in their ring slots: those that are not there (or were
// evicted by segments 1024 further on) are added to the batch's list of runs to regenerate, eight per segment.  Their
// pre-states were written by the host's bulk threads before the walker got there.
int drain_batch(fokl_dchain *e, ChainBatch &bt);

int want_resident(fokl_dchain *e, ChainBatch &bt, int &count, uint64_t first, uint64_t last)
{
    if (!e->x_ring || !e->bound) return dchain_fail(e, FOKL_ERR_STATE, "device chain: no stream is bound to the engine");
    constexpr int kRuns = FOKL_SEGMENT_BLOCKS / FOKL_PRESTATE_BLOCKS;
    constexpr size_t kRunDoubles = (size_t)FOKL_PRESTATE_BLOCKS * 312;
    const int64_t s0 = (int64_t)(first / FOKL_SEGMENT_DOUBLES), s1 = (int64_t)(last / FOKL_SEGMENT_DOUBLES);
    const int64_t published = fokl_stream_prestates_published(e->bound);
    for (int64_t sg = s0; sg <= s1; ++sg) {
        const size_t slot = (size_t)(sg % fokl::kXRingSegments);
        if (e->resident[slot] == sg) continue;
        if (sg >= published || (published - sg + 2) * kRuns > e->pre_entries)
            return dchain_fail(e, FOKL_ERR_STATE, "device chain: the pre-state of a segment is not (or no longer) in the ring");
        if (e->resident[slot] >= 0) {
            // The slot holds a segment a full ring earlier.  A batch issued before this one may still have its expansion
            // queued on another stream, reading that segment from this slot: it has to have run before the slot is
            // regenerated (residency is tracked at issue time; nothing else orders the two -- ADVICE r4).  Never seen to
            // wait: the walker would have to get 1024 segments ahead of a batch that is already on the device.
            const int64_t old = e->resident[slot];
            for (ChainBatch &other : e->batches)
                if (&other != &bt && !other.flags.empty() && other.seg_lo <= old && old <= other.seg_hi) {
                    const int rc = drain_batch(e, other);
                    if (rc != FOKL_OK) return rc;
                }
        }
        if (count + kRuns > bt.runs_cap) {
            const int cap = std::max(1024, 2 * (count + kRuns));
            fokl::SegmentArgs *grown = nullptr;
            DCHAIN_TRY(e, hipHostMalloc((void **)&grown, (size_t)cap * sizeof(fokl::SegmentArgs)));
            if (bt.h_runs) {
                std::memcpy(grown, bt.h_runs, (size_t)count * sizeof(fokl::SegmentArgs));
                (void)hipHostFree(bt.h_runs);
            }
            bt.h_runs = grown;
            bt.runs_cap = cap;
        }
        for (int run = 0; run < kRuns; ++run) {
            const int64_t entry = sg * kRuns + run;
            bt.h_runs[count].pre = e->pre_ring + (size_t)(entry % e->pre_entries) * FOKL_PRESTATE_WORDS;
            bt.h_runs[count].out = e->x_ring + slot * (size_t)FOKL_SEGMENT_DOUBLES + (size_t)run * kRunDoubles;
            ++count;
        }
        e->resident[slot] = sg;
    }
    return FOKL_OK;
}

// One batch: per job the H2D copies of its tape, then one copy of the argument records + models, the finishing kernel over
// the whole batch, one recursion launch per size class, the D2H copies of the statistics, the batch's event.
int dchain_issue(fokl_dchain *e, std::vector<ChainJob *> &batch_jobs, int batch_index)
{
    ChainBatch &bt = e->batches[batch_index];
    int64_t tp = dchain_now_ns();
    auto lap = [&](int k) { const int64_t t = dchain_now_ns(); e->ph[k] += t - tp; tp = t; };
    hipStream_t stream = e->streams[e->next_stream];
    e->next_stream = (e->next_stream + 1) % e->n_streams;
    // jobs sorted by size class so that each class is one contiguous run of argument records
    std::stable_sort(batch_jobs.begin(), batch_jobs.end(),
                     [](const ChainJob *x, const ChainJob *y) { return chain_class(x->p1) < chain_class(y->p1); });
    const size_t args_bytes = sizeof(fokl::ChainArgs) * kChainBatchMax;
    if (!bt.h_stage) {                                      // once: room for the largest batch of the largest models
        const size_t cap = args_bytes + (size_t)kChainBatchMax * 2 * 64 * kChainMaxT * sizeof(double);
        DCHAIN_TRY(e, hipHostMalloc((void **)&bt.h_stage, cap));
        bt.cap = cap;
    }
    auto *h_args = reinterpret_cast<fokl::ChainArgs *>(bt.h_stage);
    auto *h_models = reinterpret_cast<double *>(bt.h_stage + args_bytes);
    bt.flags.clear();
    bt.stream = stream;
    size_t at = 0;
    int max_blocks = 1, max_expand_blocks = 1, n_runs = 0;
    bool any_rows = false, any_arrays = false;
    lap(0);
    for (size_t n = 0; n < batch_jobs.size(); ++n) {
        ChainJob *job = batch_jobs[n];
        ChainSlot &s = e->slots[(size_t)job->slot];
        int rc = ensure_slot(e, s, job->p1, job->draws);
        if (rc) return rc;
        const int p1 = job->p1, draws = job->draws;
        double *d_gs = s.d_small, *d_gt = d_gs + draws;
        fokl::ChainArgs &args = h_args[n];
        args.rows = nullptr;
        args.x_ring = nullptr;
        if (job->rows) {
            // the device expands the rows from its own copy of the stream: the segments the tape covers must be resident
            const int rc2 = want_resident(e, bt, n_runs, job->span[0], job->span[1] + 8);
            if (rc2) return rc2;
            {
                const int64_t lo = (int64_t)(job->span[0] / FOKL_SEGMENT_DOUBLES);
                const int64_t hi = (int64_t)((job->span[1] + 8) / FOKL_SEGMENT_DOUBLES);
                if (bt.seg_hi < bt.seg_lo) {
                    bt.seg_lo = lo;
                    bt.seg_hi = hi;
                } else {
                    bt.seg_lo = std::min(bt.seg_lo, lo);
                    bt.seg_hi = std::max(bt.seg_hi, hi);
                }
            }
            args.rows = job->rows;
            args.x_ring = e->x_ring;
            args.src_normals = nullptr;
            args.src_lead = nullptr;
            args.src_gam_sig = job->gam_sig;                // read only where the walker stored a variate itself
            args.src_gam_tau = job->gam_tau;
            args.b_sig = job->astar - 1.0 / 3.0;
            args.c_sig = 1.0 / std::sqrt(9 * args.b_sig);
            args.b_tau = job->atau_star - 1.0 / 3.0;
            args.c_tau = 1.0 / std::sqrt(9 * args.b_tau);
            max_expand_blocks = std::max(max_expand_blocks, std::min(256, (draws + 3) / 4));
            any_rows = true;
        } else if (device_can_read(job->normals, (size_t)draws * p1 * sizeof(double)) &&
            device_can_read(job->gam_sig, (size_t)draws * sizeof(double)) &&
            device_can_read(job->gam_tau, (size_t)draws * sizeof(double)) &&
            (job->finished || device_can_read(job->lead, (size_t)draws * sizeof(int32_t)))) {
            // page-locked tape: the gather kernel reads it in place -- not one copy call per job
            args.src_normals = job->normals;
            args.src_gam_sig = job->gam_sig;
            args.src_gam_tau = job->gam_tau;
            args.src_lead = job->lead;
        } else {
            // ordinary memory: staged through the device (the draws' buffer holds the raw normals until the recursion,
            // which runs after the gather kernel on the same stream, overwrites it)
            double *st_gs = d_gt + draws, *st_gt = st_gs + draws;
            DCHAIN_TRY(e, hipMemcpyAsync(s.d_w, job->normals, (size_t)draws * p1 * sizeof(double), hipMemcpyHostToDevice,
                                         stream));
            DCHAIN_TRY(e, hipMemcpyAsync(st_gs, job->gam_sig, (size_t)draws * sizeof(double), hipMemcpyHostToDevice, stream));
            DCHAIN_TRY(e, hipMemcpyAsync(st_gt, job->gam_tau, (size_t)draws * sizeof(double), hipMemcpyHostToDevice, stream));
            if (!job->finished)
                DCHAIN_TRY(e, hipMemcpyAsync(s.d_lead, job->lead, (size_t)draws * sizeof(int32_t), hipMemcpyHostToDevice,
                                             stream));
            args.src_normals = s.d_w;
            args.src_gam_sig = st_gs;
            args.src_gam_tau = st_gt;
            args.src_lead = s.d_lead;
            e->staged.fetch_add(1, std::memory_order_relaxed);
        }
        if (!job->rows) {
            const int64_t total = (int64_t)draws * (p1 / 2 + 1);
            max_blocks = std::max(max_blocks, (int)std::min<int64_t>(512, (total + 255) / 256));
            any_arrays = true;
        }
        std::memcpy(h_models + at, job->model.data(), job->model.size() * sizeof(double));
        args.lamb = h_models + at;                          // page-locked: read in place, once, at the start of the chain
        args.qty = h_models + at + p1;
        at += job->model.size();
        args.normals = s.d_normals;
        args.gam_sig = d_gs;
        args.gam_tau = d_gt;
        args.w = s.d_w;
        args.stats = s.h_stats;                             // written by the recursion kernel straight into host memory
        args.b = job->b;
        args.btau = job->btau;
        args.dtd = job->dtd;
        args.sigsqd0 = job->sigsqd0;
        args.tausqd0 = job->tausqd0;
        args.ticket = (double)job->ticket;
        args.seconds_per_tick = e->seconds_per_tick;
        args.p1 = p1;
        args.draws = draws;
        args.stat_first = job->stat_first;
        args.finished = job->finished;
        bt.flags.push_back({s.h_stats + 4 + p1, job->ticket, job->slot});
        job->stream = stream;
    }
    lap(1);
    lap(2);
    const fokl::ChainArgs *d_args = h_args;
    if (any_rows) {
        // segments made on the other streams a moment ago: this stream waits for them (an event behind each stream's last
        // segment launch; what this stream made itself is ordered by the stream)
        for (int i = 0; i < kChainStreams; ++i)
            if (e->seg_recorded[i] && e->streams[i] != stream) DCHAIN_TRY(e, hipStreamWaitEvent(stream, e->seg_events[i], 0));
        if (n_runs > 0) {
            hipLaunchKernelGGL(fokl::stream_segment_kernel, dim3((unsigned)n_runs), dim3(256), 0, stream,
                               (const fokl::SegmentArgs *)bt.h_runs);
            for (int i = 0; i < kChainStreams; ++i)
                if (e->streams[i] == stream) {
                    DCHAIN_TRY(e, hipEventRecord(e->seg_events[i], stream));
                    e->seg_recorded[i] = true;
                }
            e->segments_made.fetch_add(n_runs / (FOKL_SEGMENT_BLOCKS / FOKL_PRESTATE_BLOCKS), std::memory_order_relaxed);
        }
        hipLaunchKernelGGL(fokl::tape_expand_kernel, dim3((unsigned)max_expand_blocks, (unsigned)batch_jobs.size()),
                           dim3(256), 0, stream, d_args);
    }
    if (any_arrays)
        hipLaunchKernelGGL(fokl::tape_gather_kernel, dim3((unsigned)max_blocks, (unsigned)batch_jobs.size()), dim3(256), 0,
                           stream, d_args);
    for (size_t first = 0; first < batch_jobs.size();) {
        const int cls = chain_class(batch_jobs[first]->p1);
        size_t last = first;
        while (last < batch_jobs.size() && chain_class(batch_jobs[last]->p1) == cls) ++last;
        const int count = (int)(last - first);
        switch (cls) {
        case 1: launch_chain<1>(d_args + first, count, stream, e->fast, e->segments); break;
        case 2: launch_chain<2>(d_args + first, count, stream, e->fast, e->segments); break;
        case 3: launch_chain<3>(d_args + first, count, stream, e->fast, e->segments); break;
        case 4: launch_chain<4>(d_args + first, count, stream, e->fast, e->segments); break;
        case 6: launch_chain<6>(d_args + first, count, stream, e->fast, e->segments); break;
        case 8: launch_chain<8>(d_args + first, count, stream, e->fast, e->segments); break;
        default: launch_chain<kChainMaxT>(d_args + first, count, stream, e->fast, e->segments); break;
        }
        e->launches.fetch_add(1, std::memory_order_relaxed);
        first = last;
    }
    lap(3);
    DCHAIN_TRY(e, hipGetLastError());
    lap(4);
    return FOKL_OK;
}

// 1 = the job's tape is recorded (and finished, if host threads finish it), 0 = not yet, -1 = it never will be
int tape_ready(const ChainJob *job)
{
    if (job->progress) {
        const int32_t p = __atomic_load_n(job->progress, __ATOMIC_ACQUIRE);
        if (p < 0) return -1;
        if (p < job->draws) return 0;
    }
    if (job->block_done) {
        const int nblocks = (job->draws + job->block - 1) / job->block;
        for (int blk = nblocks - 1; blk >= 0; --blk) {
            const int32_t f = __atomic_load_n(job->block_done + blk, __ATOMIC_ACQUIRE);
            if (f < 0) return -1;
            if (f == 0) return 0;
        }
    }
    return 1;
}

inline bool flag_set(const double *flag, double ticket)
{
    double seen;
    __atomic_load(flag, &seen, __ATOMIC_ACQUIRE);
    return seen == ticket;
}

// Sleep-poll a completion word.  The stream is asked now and then: work all done (or failed) without the word having
// been written means the kernel never ran to its end.
int await_flag(const double *flag, double ticket, hipStream_t stream)
{
    for (int spins = 0;; ++spins) {
        if (flag_set(flag, ticket)) return 1;
        if (spins >= 40 && spins % 20 == 0) {
            const hipError_t st = hipStreamQuery(stream);
            if (st != hipErrorNotReady) return flag_set(flag, ticket) ? 1 : -1;
        }
        std::this_thread::sleep_for(std::chrono::microseconds(spins < 40 ? 20 : 50));
    }
}

// Waits until every job of the launch this batch record was last used for has stored its ticket.  A job whose slot has
// since been given to a later job was released, hence had run: its word holds that job's ticket (or the reset value) by now.
int drain_batch(fokl_dchain *e, ChainBatch &bt)
{
    for (const auto &f : bt.flags) {
        {
            std::lock_guard<std::mutex> lock(e->m);
            if (e->slots[(size_t)f.slot].ticket != f.ticket) continue;
        }
        if (await_flag(f.word, (double)f.ticket, bt.stream) < 0) break;  // a failed launch: its waiters report it
    }
    bt.flags.clear();
    bt.seg_lo = 0;
    bt.seg_hi = -1;
    return FOKL_OK;
}

// A batch record whose previous launch has run: the kernels read its staging area in place, so it may only be rewritten
// once every job of that launch has stored its ticket (records are taken in rotation).
int take_batch_record(fokl_dchain *e)
{
    ChainBatch &bt = e->batches[e->next_batch];
    (void)drain_batch(e, bt);
    const int index = e->next_batch;
    e->next_batch = (e->next_batch + 1) % kChainBatches;
    return index;
}

// CPU time of every engine's dispatcher thread so far (fokl_thread_cpu_seconds): finished ones + the live ones' clocks
std::atomic<int64_t> g_dispatch_cpu_done_ns{0};
std::mutex g_dispatch_m;
std::vector<pthread_t> g_dispatchers;

void dchain_dispatch(fokl_dchain *e)
{
    {
        std::lock_guard<std::mutex> lock(g_dispatch_m);
        g_dispatchers.push_back(pthread_self());
    }
    struct Note {
        ~Note()
        {
            std::lock_guard<std::mutex> lock(g_dispatch_m);
            timespec ts;
            if (clock_gettime(CLOCK_THREAD_CPUTIME_ID, &ts) == 0)
                g_dispatch_cpu_done_ns.fetch_add((int64_t)ts.tv_sec * 1000000000LL + ts.tv_nsec);
            for (size_t i = 0; i < g_dispatchers.size(); ++i)
                if (pthread_equal(g_dispatchers[i], pthread_self())) {
                    g_dispatchers.erase(g_dispatchers.begin() + (std::ptrdiff_t)i);
                    break;
                }
        }
    } note;
    (void)hipSetDevice(e->device);
    std::vector<ChainJob *> ready;
    for (;;) {
        ready.clear();
        bool failed_head = false;
        int64_t wait_ns = 0;
        {
            std::unique_lock<std::mutex> lock(e->m);
            e->cv_queue.wait(lock, [&] { return e->stop || !e->queue.empty(); });
            if (e->queue.empty()) return;                   // stop requested and the queue is drained
            // jobs from the front whose tapes are there; a batch goes out when it is full enough, when its oldest job
            // has waited long enough, or when somebody waits for a result (flush)
            const int64_t now = dchain_now_ns();
            size_t n = 0;
            int head_state = 1;
            while (n < e->queue.size() && (int)n < kChainBatchMax) {
                const int st = tape_ready(e->queue[n]);
                if (st != 1) {
                    if (n == 0) head_state = st;
                    break;
                }
                ++n;
            }
            if (head_state < 0) {
                ChainJob *job = e->queue.front();
                e->queue.pop_front();
                job->status = FOKL_ERR_STATE;
                job->error = "device chain: the noise tape producer failed or the tape was sent back";
                job->state = 2;
                failed_head = true;
            } else {
                const int64_t age = n > 0 ? now - e->queue.front()->t_submit : 0;
                const bool due = n > 0 && ((int)n >= e->batch_target || e->flush > 0 || e->stop ||
                                           age >= e->batch_delay_ns);
                if (n > 0 && !due && n == e->queue.size()) wait_ns = e->batch_delay_ns - age;
                if (due) {
                    ready.assign(e->queue.begin(), e->queue.begin() + (std::ptrdiff_t)n);
                    e->queue.erase(e->queue.begin(), e->queue.begin() + (std::ptrdiff_t)n);
                    if (e->flush > 0 && e->queue.empty()) e->flush = 0;
                }
            }
        }
        if (failed_head) {
            e->cv_state.notify_all();
            continue;
        }
        if (ready.empty()) {
            if (wait_ns > 0) {                              // tapes are there, the batch is young: until it is due or grows
                std::unique_lock<std::mutex> lock(e->m);
                const size_t seen = e->queue.size();
                e->cv_queue.wait_for(lock, std::chrono::nanoseconds(wait_ns),
                                     [&] { return e->stop || e->flush > 0 || e->queue.size() != seen; });
            } else {                                        // the head's tape is still on record: poll its progress flag
                std::this_thread::sleep_for(std::chrono::microseconds(25));
            }
            continue;
        }
        const int index = take_batch_record(e);             // may sleep until an earlier batch has run
        const int64_t t0 = dchain_now_ns();
        int rc = dchain_issue(e, ready, index);
        const std::string err = rc == FOKL_OK ? std::string() : e->err;
        e->busy_ns.fetch_add(dchain_now_ns() - t0, std::memory_order_relaxed);
        {
            std::lock_guard<std::mutex> lock(e->m);
            for (ChainJob *job : ready) {
                job->status = rc;
                job->error = err;
                job->state = rc == FOKL_OK ? 1 : 2;
            }
            if (rc == FOKL_OK) e->issued.fetch_add((int64_t)ready.size(), std::memory_order_relaxed);
        }
        e->cv_state.notify_all();
    }
}

// -> the job once the dispatcher has dealt with it (issued or failed); nullptr + error for an unknown ticket
ChainJob *dchain_settled(fokl_dchain *e, int64_t ticket, int *rc)
{
    std::unique_lock<std::mutex> lock(e->m);
    auto it = e->jobs.find(ticket);
    if (it == e->jobs.end()) {
        *rc = dchain_fail(e, FOKL_ERR_ARG, "device chain: unknown or released ticket");
        return nullptr;
    }
    ChainJob *job = it->second;
    if (job->state == 0) {
        e->flush += 1;                                      // do not let it sit in a half-full batch
        e->cv_queue.notify_all();
        e->cv_state.wait(lock, [&] { return job->state != 0; });
    }
    if (job->state == 2) {
        *rc = dchain_fail(e, job->status, job->error);
        return nullptr;
    }
    *rc = FOKL_OK;
    return job;
}

// The job has run: the recursion kernel's last store is the job's ticket behind its statistics.  The first caller to see
// that also reads the job's fallback indicator (the slot is the job's until it is released) into the engine's counter.
int dchain_complete(fokl_dchain *e, ChainJob *job, bool block)
{
    const double *stats = e->slots[(size_t)job->slot].h_stats;
    const double *flag = stats + 4 + job->p1;
    int ran = flag_set(flag, (double)job->ticket) ? 1 : 0;
    if (!ran && block) ran = await_flag(flag, (double)job->ticket, job->stream);
    if (ran == 1 && !job->counted.exchange(true, std::memory_order_relaxed) && stats[6 + job->p1] != 0.0)
        e->recuts.fetch_add(1, std::memory_order_relaxed);
    return ran;
}

// A job with the fields both ways of handing over a tape share; the caller adds the tape itself.
ChainJob *new_job(int p1, int draws, int stat_first, const double *lamb, const double *qty, double b, double btau, double dtd,
                  double sigsqd0, double tausqd0, const double *gam_sig, const double *gam_tau, const int32_t *progress)
{
    auto *job = new ChainJob();
    job->p1 = p1;
    job->draws = draws;
    job->stat_first = stat_first;
    job->b = b;
    job->btau = btau;
    job->dtd = dtd;
    job->sigsqd0 = sigsqd0;
    job->tausqd0 = tausqd0;
    job->model.assign(lamb, lamb + p1);
    job->model.insert(job->model.end(), qty, qty + p1);
    job->gam_sig = gam_sig;
    job->gam_tau = gam_tau;
    job->progress = progress;
    job->t_submit = dchain_now_ns();
    return job;
}

// Takes the job over (it is deleted on failure): a free slot, the slot's statistics area with its completion word cleared,
// the job's ticket, and the job into the dispatcher's queue.  who: the entry point, for the error text.
int enqueue_job(fokl_dchain *e, ChainJob *job, const char *who, int64_t *ticket, const double **stats_area)
{
    {
        std::lock_guard<std::mutex> lock(e->m);
        for (size_t i = 0; i < e->slots.size(); ++i)
            if (!e->slots[i].busy) {
                job->slot = (int)i;
                break;
            }
        if (job->slot < 0) {
            delete job;
            return dchain_fail(e, FOKL_ERR_STATE, std::string(who) + ": every slot holds a chain that was not released");
        }
        ChainSlot &slot = e->slots[(size_t)job->slot];
        if (ensure_stats(e, slot, job->p1) != FOKL_OK) {    // (allocated once per slot, for the largest model)
            delete job;
            return FOKL_ERR_HIP;
        }
        slot.busy = true;
        job->ticket = e->next_ticket++;
        slot.ticket = job->ticket;
        __atomic_store_n(reinterpret_cast<int64_t *>(slot.h_stats + 4 + job->p1), (int64_t)0, __ATOMIC_RELEASE);
        e->jobs[job->ticket] = job;
        e->queue.push_back(job);
        *ticket = job->ticket;
        if (stats_area) *stats_area = slot.h_stats;
    }
    e->cv_queue.notify_one();
    return FOKL_OK;
}

}  // namespace

extern "C" __attribute__((visibility("hidden"))) int64_t fokl_dchain_dispatcher_cpu_ns()
{
    std::lock_guard<std::mutex> lock(g_dispatch_m);
    int64_t total = g_dispatch_cpu_done_ns.load();
    for (pthread_t t : g_dispatchers) {
        clockid_t cid;
        timespec ts;
        if (pthread_getcpuclockid(t, &cid) == 0 && clock_gettime(cid, &ts) == 0)
            total += (int64_t)ts.tv_sec * 1000000000LL + ts.tv_nsec;
    }
    return total;
}

extern "C" int fokl_dchain_create(int device, int slots, fokl_dchain **out)
{
    if (!out || slots < 1 || slots > 4096) return dchain_fail(nullptr, FOKL_ERR_ARG, "fokl_dchain_create: bad argument");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count)
        return dchain_fail(nullptr, FOKL_ERR_HIP, "fokl_dchain_create: no such HIP device");
    auto *e = new fokl_dchain();
    e->device = device;
    e->slots.resize((size_t)slots);
    if (hipSetDevice(device) != hipSuccess) {
        delete e;
        return dchain_fail(nullptr, FOKL_ERR_HIP, "fokl_dchain_create: hipSetDevice failed");
    }
    for (int i = 0; i < kChainStreams; ++i)
        if (hipStreamCreateWithFlags(&e->streams[i], hipStreamNonBlocking) != hipSuccess) {
            for (int j = 0; j < i; ++j) (void)hipStreamDestroy(e->streams[j]);
            delete e;
            return dchain_fail(nullptr, FOKL_ERR_HIP, "fokl_dchain_create: hipStreamCreate failed");
        }
    int khz = 0;
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device) == hipSuccess && khz > 0)
        e->seconds_per_tick = 1e-3 / (double)khz;
    if (const char *v = std::getenv("FOKL_DCHAIN_RECURSION")) {
        e->fast = std::strcmp(v, "exact") != 0;
        e->segments = std::strcmp(v, "serial") != 0;
    }
    if (const char *v = std::getenv("FOKL_DCHAIN_STREAMS")) e->n_streams = std::max(1, std::min(kChainStreams, std::atoi(v)));
    if (const char *v = std::getenv("FOKL_DCHAIN_BATCH")) e->batch_target = std::max(1, std::min(kChainBatchMax, std::atoi(v)));
    if (const char *v = std::getenv("FOKL_DCHAIN_DELAY_US")) e->batch_delay_ns = 1000LL * std::max(0, std::atoi(v));
    e->dispatcher = std::thread(dchain_dispatch, e);
    *out = e;
    return FOKL_OK;
}

extern "C" void fokl_dchain_destroy(fokl_dchain *e)
{
    if (!e) return;
    {
        std::lock_guard<std::mutex> lock(e->m);
        e->stop = true;
    }
    e->cv_queue.notify_all();
    if (e->dispatcher.joinable()) e->dispatcher.join();
    if (std::getenv("FOKL_DCHAIN_TRACE"))
        std::fprintf(stderr, "dchain phases ms: prep %.2f jobs %.2f args-copy %.2f launches %.2f event %.2f | issued %lld launches %lld\n",
                     e->ph[0] / 1e6, e->ph[1] / 1e6, e->ph[2] / 1e6, e->ph[3] / 1e6, e->ph[4] / 1e6,
                     (long long)e->issued.load(), (long long)e->launches.load());
    (void)hipSetDevice(e->device);
    for (auto &st : e->streams)
        if (st) (void)hipStreamSynchronize(st);
    for (auto &kv : e->jobs) delete kv.second;
    for (auto &s : e->slots) {
        if (s.d_normals) (void)hipFree(s.d_normals);
        if (s.d_w) (void)hipFree(s.d_w);
        if (s.d_small) (void)hipFree(s.d_small);
        if (s.d_lead) (void)hipFree(s.d_lead);
        if (s.h_stats) (void)hipHostFree(s.h_stats);
    }
    for (auto &bt : e->batches) {
        if (bt.h_stage) (void)hipHostFree(bt.h_stage);
        if (bt.h_runs) (void)hipHostFree(bt.h_runs);
    }
    if (e->x_ring) (void)hipFree(e->x_ring);
    if (e->pre_ring) (void)hipHostFree(e->pre_ring);
    for (auto &ev : e->seg_events)
        if (ev) (void)hipEventDestroy(ev);
    for (auto &st : e->streams)
        if (st) (void)hipStreamDestroy(st);
    delete e;
}

extern "C" int fokl_dchain_submit(fokl_dchain *e, int p1, int draws, const double *lamb, const double *qty, double b,
                                  double btau, double dtd, double sigsqd0, double tausqd0, const double *normals,
                                  const int32_t *lead, const double *gam_sig, const double *gam_tau,
                                  const int32_t *progress, const int32_t *block_done, int block, int finished,
                                  int stat_first, int64_t *ticket, const double **stats_area)
{
    if (!e || !lamb || !qty || !normals || !lead || !gam_sig || !gam_tau || !ticket || p1 <= 0 || draws < 0 ||
        stat_first < 0 || (block_done && block < 1))
        return dchain_fail(e, FOKL_ERR_ARG, "fokl_dchain_submit: null pointer, empty model or bad block size");
    if (p1 > 64 * kChainMaxT)
        return dchain_fail(e, FOKL_ERR_ARG, "fokl_dchain_submit: more columns than the device chain handles (768)");
    ChainJob *job = new_job(p1, draws, stat_first, lamb, qty, b, btau, dtd, sigsqd0, tausqd0, gam_sig, gam_tau, progress);
    job->finished = finished ? 1 : 0;
    job->normals = normals;
    job->lead = lead;
    job->block_done = block_done;
    job->block = block;
    return enqueue_job(e, job, "fokl_dchain_submit", ticket, stats_area);
}

// The page-locked ring the host's bulk threads leave the stream's pre-states in (fokl_stream_create / fokl_pool_create),
// and -- first call -- the device ring of regenerated segments (654 MB).
extern "C" int fokl_dchain_prestate_ring(fokl_dchain *e, uint32_t **ring, int *entries)
{
    if (!e || !ring || !entries) return dchain_fail(e, FOKL_ERR_ARG, "fokl_dchain_prestate_ring: null pointer");
    if (!e->pre_ring) {
        DCHAIN_TRY(e, hipSetDevice(e->device));
        const int count = 8192;                             // 1024 segments' worth of runs (20 MB): as many as x_ring holds
        void *p = nullptr;
        DCHAIN_TRY(e, hipHostMalloc(&p, (size_t)count * FOKL_PRESTATE_WORDS * sizeof(uint32_t), hipHostMallocDefault));
        e->pre_ring = static_cast<uint32_t *>(p);
        e->pre_entries = count;
        bool ok = hipMalloc((void **)&e->x_ring, (size_t)fokl::kXRingSegments * FOKL_SEGMENT_DOUBLES * sizeof(double)) == hipSuccess;
        for (int i = 0; ok && i < kChainStreams; ++i)
            ok = hipEventCreateWithFlags(&e->seg_events[i], hipEventDisableTiming) == hipSuccess;
        if (!ok) {
            (void)hipHostFree(e->pre_ring);
            e->pre_ring = nullptr;
            e->x_ring = nullptr;
            return dchain_fail(e, FOKL_ERR_HIP, "fokl_dchain_prestate_ring: no device memory for the stream's segments");
        }
        e->resident.assign((size_t)fokl::kXRingSegments, -1);
    }
    *ring = e->pre_ring;
    *entries = e->pre_entries;
    return FOKL_OK;
}

// The stream whose pre-states the ring receives from now on (created with the ring); NULL: none.  Every chain of the
// stream bound before must have run.
extern "C" int fokl_dchain_bind_stream(fokl_dchain *e, const fokl_stream *stream)
{
    if (!e) return dchain_fail(e, FOKL_ERR_ARG, "fokl_dchain_bind_stream: null engine");
    std::lock_guard<std::mutex> lock(e->m);
    if (!e->queue.empty()) return dchain_fail(e, FOKL_ERR_STATE, "fokl_dchain_bind_stream: chains of the stream bound before are queued");
    e->bound = stream;
    std::fill(e->resident.begin(), e->resident.end(), (int64_t)-1);
    for (auto &r : e->seg_recorded) r = false;
    return FOKL_OK;
}

// fokl_dchain_submit for a tape that exists as ROWS only (fokl_pool_submit_noise with finish == 2, on the stream bound to
// the engine): rows [draws] and gam_sig / gam_tau [draws] (read only where the walker stored a variate itself) in
// page-locked memory; span [2] as fokl_pool_submit_noise fills it; astar / atau_star as given to the walk.
extern "C" int fokl_dchain_submit_rows(fokl_dchain *e, int p1, int draws, const double *lamb, const double *qty, double b,
                                       double btau, double dtd, double sigsqd0, double tausqd0, double astar,
                                       double atau_star, const fokl_tape_row *rows, const double *gam_sig,
                                       const double *gam_tau, const int32_t *progress, const uint64_t *span, int stat_first,
                                       int64_t *ticket, const double **stats_area)
{
    if (!e || !lamb || !qty || !rows || !gam_sig || !gam_tau || !progress || !span || !ticket || p1 <= 0 || draws < 0 ||
        stat_first < 0 || !(astar > 1.0) || !(atau_star > 1.0))
        return dchain_fail(e, FOKL_ERR_ARG, "fokl_dchain_submit_rows: null pointer, empty model or gamma shape <= 1");
    if (p1 > 64 * kChainMaxT)
        return dchain_fail(e, FOKL_ERR_ARG, "fokl_dchain_submit_rows: more columns than the device chain handles (768)");
    if (!e->x_ring || !e->bound) return dchain_fail(e, FOKL_ERR_STATE, "fokl_dchain_submit_rows: no stream is bound to the engine");
    if (!device_can_read(rows, (size_t)draws * sizeof(fokl_tape_row)) || !device_can_read(gam_sig, (size_t)draws * sizeof(double)) ||
        !device_can_read(gam_tau, (size_t)draws * sizeof(double)))
        return dchain_fail(e, FOKL_ERR_ARG, "fokl_dchain_submit_rows: the rows must lie in page-locked memory (fokl_host_alloc)");
    ChainJob *job = new_job(p1, draws, stat_first, lamb, qty, b, btau, dtd, sigsqd0, tausqd0, gam_sig, gam_tau, progress);
    job->astar = astar;
    job->atau_star = atau_star;
    job->rows = rows;
    job->span = span;
    const int rc = enqueue_job(e, job, "fokl_dchain_submit_rows", ticket, stats_area);
    if (rc == FOKL_OK) e->rows_jobs.fetch_add(1, std::memory_order_relaxed);
    return rc;
}

extern "C" int fokl_dchain_stream_stats(fokl_dchain *e, int64_t *segments_made, int64_t *rows_jobs)
{
    if (!e) return dchain_fail(nullptr, FOKL_ERR_ARG, "fokl_dchain_stream_stats: null engine");
    if (segments_made) *segments_made = e->segments_made.load(std::memory_order_relaxed);
    if (rows_jobs) *rows_jobs = e->rows_jobs.load(std::memory_order_relaxed);
    return FOKL_OK;
}

// Issue what is queued now instead of waiting for the batch to fill or age (the caller knows that nothing more is coming
// for a while: the end of a sub-stage's kill tests, the end of a fit).
extern "C" int fokl_dchain_flush(fokl_dchain *e)
{
    if (!e) return dchain_fail(nullptr, FOKL_ERR_ARG, "fokl_dchain_flush: null engine");
    {
        std::lock_guard<std::mutex> lock(e->m);
        if (e->queue.empty()) return FOKL_OK;
        e->flush += 1;
    }
    e->cv_queue.notify_all();
    return FOKL_OK;
}

extern "C" int fokl_dchain_poll(fokl_dchain *e, int64_t ticket)
{
    if (!e) return 0;
    ChainJob *job = nullptr;
    {
        std::lock_guard<std::mutex> lock(e->m);
        auto it = e->jobs.find(ticket);
        if (it == e->jobs.end()) return 1;                  // nothing to wait for
        job = it->second;
        if (job->state == 0) return 0;
        if (job->state == 2) return 1;                      // wait() reports the failure
    }
    return dchain_complete(e, job, false) != 0 ? 1 : 0;
}

extern "C" int fokl_dchain_wait(fokl_dchain *e, int64_t ticket, double *stats_out)
{
    if (!e || !stats_out) return dchain_fail(e, FOKL_ERR_ARG, "fokl_dchain_wait: null pointer");
    int rc = FOKL_OK;
    ChainJob *job = dchain_settled(e, ticket, &rc);
    if (!job) return rc;
    if (dchain_complete(e, job, true) < 0) return dchain_fail(e, FOKL_ERR_HIP, "fokl_dchain_wait: the chain's kernel did not run to its end");
    std::memcpy(stats_out, e->slots[(size_t)job->slot].h_stats, (size_t)(4 + job->p1) * sizeof(double));
    return FOKL_OK;
}

extern "C" int fokl_dchain_fetch_w(fokl_dchain *e, int64_t ticket, double *w_out)
{
    if (!e || !w_out) return dchain_fail(e, FOKL_ERR_ARG, "fokl_dchain_fetch_w: null pointer");
    int rc = FOKL_OK;
    ChainJob *job = dchain_settled(e, ticket, &rc);
    if (!job) return rc;
    ChainSlot &s = e->slots[(size_t)job->slot];
    DCHAIN_TRY(e, hipSetDevice(e->device));
    if (dchain_complete(e, job, true) < 0) return dchain_fail(e, FOKL_ERR_HIP, "fokl_dchain_fetch_w: the chain's kernel did not run to its end");
    DCHAIN_TRY(e, hipMemcpy(w_out, s.d_w, (size_t)job->draws * job->p1 * sizeof(double), hipMemcpyDeviceToHost));
    return FOKL_OK;
}

extern "C" int fokl_dchain_release(fokl_dchain *e, int64_t ticket)
{
    if (!e) return dchain_fail(nullptr, FOKL_ERR_ARG, "fokl_dchain_release: null engine");
    {
        std::lock_guard<std::mutex> lock(e->m);
        if (e->jobs.find(ticket) == e->jobs.end()) return FOKL_OK;     // idempotent
    }
    int rc = FOKL_OK;
    ChainJob *job = dchain_settled(e, ticket, &rc);                     // its host buffers are in use until it is issued
    if (job) (void)dchain_complete(e, job, true);                       // ... and until the copies out of them have run
    {
        std::lock_guard<std::mutex> lock(e->m);
        auto it = e->jobs.find(ticket);
        if (it == e->jobs.end()) return FOKL_OK;
        job = it->second;
        e->jobs.erase(it);
        e->slots[(size_t)job->slot].busy = false;
    }
    delete job;
    return FOKL_OK;
}

// 1 = released (or unknown: released before), 0 = the chain has not run yet -- nothing is waited for.
extern "C" int fokl_dchain_try_release(fokl_dchain *e, int64_t ticket)
{
    if (!e) return 1;
    ChainJob *job = nullptr;
    {
        std::lock_guard<std::mutex> lock(e->m);
        auto it = e->jobs.find(ticket);
        if (it == e->jobs.end()) return 1;
        job = it->second;
        if (job->state == 0) return 0;
    }
    if (job->state == 1 && dchain_complete(e, job, false) == 0) return 0;
    {
        std::lock_guard<std::mutex> lock(e->m);
        e->jobs.erase(ticket);
        e->slots[(size_t)job->slot].busy = false;
    }
    delete job;
    return 1;
}

extern "C" int fokl_dchain_stats(fokl_dchain *e, double *busy_seconds, int64_t *issued, int64_t *launches,
                                 int64_t *staged)
{
    if (!e) return dchain_fail(nullptr, FOKL_ERR_ARG, "fokl_dchain_stats: null engine");
    if (busy_seconds) *busy_seconds = 1e-9 * (double)e->busy_ns.load(std::memory_order_relaxed);
    if (issued) *issued = e->issued.load(std::memory_order_relaxed);
    if (launches) *launches = e->launches.load(std::memory_order_relaxed);
    if (staged) *staged = e->staged.load(std::memory_order_relaxed);
    return FOKL_OK;
}

extern "C" int fokl_dchain_recuts(fokl_dchain *e, int64_t *recuts)
{
    if (!e || !recuts) return dchain_fail(e, FOKL_ERR_ARG, "fokl_dchain_recuts: null pointer");
    *recuts = e->recuts.load(std::memory_order_relaxed);
    return FOKL_OK;
}

extern "C" int fokl_host_alloc(size_t bytes, void **out)
{
    if (!out || bytes == 0) return dchain_fail(nullptr, FOKL_ERR_ARG, "fokl_host_alloc: null pointer or empty request");
    *out = nullptr;
    hipError_t rc = hipHostMalloc(out, bytes, hipHostMallocDefault);
    if (rc != hipSuccess) return dchain_fail(nullptr, FOKL_ERR_HIP, std::string("hipHostMalloc: ") + hipGetErrorString(rc));
    std::lock_guard<std::mutex> lock(g_pinned_mutex);
    g_pinned_blocks[reinterpret_cast<uintptr_t>(*out)] = bytes;
    return FOKL_OK;
}

extern "C" int fokl_host_free(void *ptr)
{
    if (!ptr) return FOKL_OK;
    {
        std::lock_guard<std::mutex> lock(g_pinned_mutex);
        g_pinned_blocks.erase(reinterpret_cast<uintptr_t>(ptr));
    }
    if (hipHostFree(ptr) != hipSuccess) return dchain_fail(nullptr, FOKL_ERR_HIP, "hipHostFree failed");
    return FOKL_OK;
}

// G2 on the device (textually included by fokl_hip.hip): the eigen-decomposition of a candidate's XtX sub-block
// (FoKLRoutines.py:1499, scipy.linalg.eigh) and what hangs on it -- Q'Xty, betahat (FR:1502-1504), the residual moments
// of y - X betahat from the Gram alone (SURVEY A.4) -- for models of up to FOKL_DSPECTRAL_MAX_COLUMNS columns.  Up to
// round 3 every one of the ~400 decompositions of a headline fit was a LAPACK dsyevr call on a host thread (0.42 ms each
// at 66 columns, 1.2 ms at 140: 0.17 CPU-seconds of a 0.30 CPU-second fit, eight threads busy through the kill tests).
//
// Cyclic two-sided Jacobi in the parallel (round-robin tournament) ordering -- a round rotates m / 2 disjoint index pairs
// at once -- split in two kernels, because only the MATRIX half of the iteration is sequential:
//
//   spectral_sweep_kernel     one workgroup per matrix, the matrix (packed lower triangle) in LDS.  Per round: (1) one
//                             lane per pair forms its rotation from (a_pp, a_qq, a_pq) and writes the pair's own 2 x 2
//                             block; (2) every lane applies J_a' X J_b to one 2 x 2 block per unordered pair of pairs.
//                             Two barriers per round, m - 1 rounds per sweep, sweeps until |a_pq| <= 2^-53 sqrt(a_pp
//                             a_qq) for every pair (the relative criterion of Demmel & Veselic for positive definite
//                             matrices: eigenvalues and eigenvectors to the accuracy the DATA determine them, which
//                             dsyevr's MRRR does not promise).  The rotations (c, s) of every round that rotated anything
//                             are logged to device memory.
//   spectral_vectors_kernel   V' <- J' V' column by column: column i of V' (= row i of V) only ever meets column i, so
//                             every column is its own problem once the rotations are known -- one WAVEFRONT per column
//                             replays the log on its n numbers in LDS, lane k taking pair k of each round; no barriers.
//                             The workgroup that finishes a matrix last (a counter in device memory) completes the job:
//                             eigenvalues ascending (LAPACK's order), the sign convention of engine.eigh_canonical,
//                             Q'Xty, betahat, the moments in double-double arithmetic (the host path uses 80-bit long
//                             double there), all stored straight into the job's page-locked result area, the ticket
//                             last with system-wide release semantics.
//
// Jacobi's eigenvectors are not dsyevr's bit for bit: both are within the conditioning of the eigenvectors (eps ||XtX|| /
// gap) of the exact ones, Jacobi closer (profiles/eigh_device_r04.txt: 1e-14 .. 1e-11 of the draw map's scale against
// dsyevr's 1e-12 .. 4e-11).  What the product returns moves by that much -- the amount by which dsyevr's own output moves
// when the last bits of XtX do (DESIGN section 6) -- the selected model and every kill-test decision of the goldens do not.
namespace fokl {

typedef double spectral_d2 __attribute__((ext_vector_type(2)));        // (c, s): a native vector, storable through any address space

struct SpectralHeader {             // device memory, one per job in flight
    int logged;                     // rounds in the log
    int arrived;                    // workgroups of the vectors kernel that have finished
    int sweeps, rotations, converged, pad;
    long long t_begin;              // wall_clock64 when the sweep kernel took the job
};

struct SpectralArgs {
    const double *in;               // page-locked: a, packed lower triangle [n (n + 1) / 2] | xty [n] | ones [n] | ones_y | yty
    double *out;                    // page-locked: lamb [n] | qty [n] | betahat [n] | Qt [n][n] | moments [2] |
                                    //              info [4] = sweeps, rotations, seconds, not converged | ticket
    // the job's work area (device memory)
    double *d_a;                    // [n (n + 1) / 2] the block as it came (packed lower triangle)
    double *d_vt;                   // [n][n] V' after the last rotation
    double *d_lam;                  // [n] diagonal after the last rotation
    spectral_d2 *d_log;                 // [log_rounds][h] (c, s) of every logged round
    int *d_log_round;               // [log_rounds] its round number within a sweep
    SpectralHeader *d_hdr;
    double ticket, seconds_per_tick;
    int n, canonical, log_rounds, pad;
};

constexpr int kSpectralMaxColumns = FOKL_DSPECTRAL_MAX_COLUMNS;
constexpr int kSpectralMaxPairs = (kSpectralMaxColumns + 1) / 2;
constexpr int kSpectralMaxSweeps = 30;
constexpr int kSpectralLogSweeps = 16;                      // log capacity in sweeps' worth of rounds
constexpr int kSpectralBlocksPerLane = 5;                   // 96 pairs: 48 * 95 blocks over 1024 lanes
constexpr int kSpectralColumnsPerGroup = 4;                 // wavefronts (= columns) per workgroup of the vectors kernel

// double-double helpers (error-free transformations; fma is exact on this hardware)
struct dd {
    double hi, lo;
};
__device__ __forceinline__ dd dd_two_sum(double a, double b)
{
    const double s = a + b, bb = s - a;
    return {s, (a - (s - bb)) + (b - bb)};
}
__device__ __forceinline__ dd dd_add(dd x, dd y)
{
    dd s = dd_two_sum(x.hi, y.hi);
    const dd t = dd_two_sum(x.lo, y.lo);
    s.lo += t.hi;
    s = dd_two_sum(s.hi, s.lo);
    s.lo += t.lo;
    return dd_two_sum(s.hi, s.lo);
}
__device__ __forceinline__ dd dd_mul_d(dd x, double y)
{
    const double p = x.hi * y;
    const double e = __builtin_fma(x.hi, y, -p) + x.lo * y;
    return dd_two_sum(p, e);
}
__device__ __forceinline__ dd dd_prod(double x, double y)
{
    const double p = x * y;
    return {p, __builtin_fma(x, y, -p)};
}

// Global-memory accesses spelled as such: through a generic pointer they become FLAT instructions, which count on the
// LDS counter too -- the s_waitcnt lgkmcnt(0) in front of every barrier then waits for a store to be acknowledged by
// memory (the sweep kernel's log stores: 1 us per round, two thirds of the kernel).
typedef __attribute__((address_space(1))) spectral_d2 *spectral_g2_ptr;
typedef __attribute__((address_space(1))) const spectral_d2 *spectral_cg2_ptr;
typedef __attribute__((address_space(1))) int *spectral_gi_ptr;
typedef __attribute__((address_space(1))) const int *spectral_cgi_ptr;
__device__ __forceinline__ void gstore2(spectral_d2 *p, spectral_d2 v) { *(spectral_g2_ptr)(p) = v; }
__device__ __forceinline__ spectral_d2 gload2(const spectral_d2 *p) { return *(spectral_cg2_ptr)(p); }
__device__ __forceinline__ void gstore_i(int *p, int v) { *(spectral_gi_ptr)(p) = v; }
__device__ __forceinline__ int gload_i(const int *p) { return *(spectral_cgi_ptr)(p); }

// round r of a sweep pairs index m - 1 with r, and (r + k) mod (m - 1) with (r - k) mod (m - 1) for k = 1 .. m / 2 - 1
__device__ __forceinline__ void spectral_pair(int r, int k, int m1, int &p, int &q)
{
    if (k == 0) {
        p = m1;
        q = r;
    } else {
        p = r + k;
        if (p >= m1) p -= m1;
        q = r - k;
        if (q < 0) q += m1;
    }
}

// packed lower triangle: (i, j) and (j, i) are one number
__device__ __forceinline__ int spectral_at(int i, int j)
{
    const int hi = max(i, j), lo = min(i, j);
    return (__mul24(hi, hi + 1) >> 1) + lo;                 // (24-bit multiply: full rate, the 32-bit one is not)
}

// 1 / x and 1 / sqrt(x) for normal, positive x to an ulp or two: the hardware's seed (about 2^-27 relative) and two Newton
// steps, a third of the dependent instructions of IEEE division and square root -- the rotation lane's chain of four
// such operations is the critical path of every round.  (A rotation needs c^2 + s^2 = 1 to rounding, not correctly
// rounded c and s.)
__device__ __forceinline__ double spectral_rcp(double x)
{
    double y = __builtin_amdgcn_rcp(x);
    y = __builtin_fma(__builtin_fma(-x, y, 1.0), y, y);
    y = __builtin_fma(__builtin_fma(-x, y, 1.0), y, y);
    return y;
}
__device__ __forceinline__ double spectral_rsqrt(double x)
{
    double y = __builtin_amdgcn_rsq(x);
    // y <- y + y (1 - x y^2) / 2, twice
    double e = __builtin_fma(-x * y, y, 1.0);
    y = __builtin_fma(0.5 * y, e, y);
    e = __builtin_fma(-x * y, y, 1.0);
    y = __builtin_fma(0.5 * y, e, y);
    return y;
}

__global__ __launch_bounds__(1024) void spectral_sweep_kernel(const SpectralArgs *__restrict__ jobs)
{
    extern __shared__ double spectral_lds[];
    __shared__ double rot_c[kSpectralMaxPairs], rot_s[kSpectralMaxPairs];
    __shared__ int rotated[3], round_active[2];
    const SpectralArgs a = jobs[blockIdx.x];
    const int tid = threadIdx.x, nthreads = blockDim.x;
    const int n = a.n, m = (n + 1) & ~1, h = m >> 1, m1 = m - 1;
    double *A = spectral_lds;
    const double *in = a.in;
    if (tid == 0) {
        a.d_hdr->t_begin = wall_clock64();                  // the clock of the whole job (the vectors kernel stops it)
        a.d_hdr->arrived = 0;
    }

    // ---- load: the caller's block, lower triangle (dsyevr is called with uplo = 'L') packed row by row -- the layout the
    // matrix has in LDS, read in one dense sweep (element by element out of a square block in page-locked memory the bus
    // served 8 bytes at a time: 0.4 of the 0.57 ms of a 66-column job).  An odd n gets an isolated dummy index (diagonal
    // 1, never rotated).  A copy goes to device memory for the residual moments.
    const int packed = (n * (n + 1)) >> 1;
    for (int t = tid; t < packed; t += nthreads) {
        const double v = gload(in + t);
        A[t] = v;
        gstore(a.d_a + t, v);
    }
    if (m > n)
        for (int j = tid; j < m; j += nthreads) A[packed + j] = j == n ? 1.0 : 0.0;
    if (tid < 3) rotated[tid] = 0;
    if (tid < 2) round_active[tid] = 0;

    // ---- this lane's share of every round: off-diagonal blocks (pairs a < b).  The triangle a < b is folded so that
    // item -> (a, b) needs one division, done once.  (Constant indices only: the arrays live in registers.)
    int blk_a[kSpectralBlocksPerLane], blk_b[kSpectralBlocksPerLane];
    {
        const int per_row = max(h - 1, 1), rows_f = (h + 1) >> 1, total = h > 1 ? rows_f * per_row : 0;
#pragma unroll
        for (int e = 0; e < kSpectralBlocksPerLane; ++e) {
            const int id = tid + e * nthreads;
            blk_a[e] = -1;
            blk_b[e] = 0;
            if (id >= total) continue;
            const int f = id / per_row, c = id - f * per_row;
            if (c < h - 1 - f) {
                blk_a[e] = f;
                blk_b[e] = f + 1 + c;
            } else if (h - 1 - f != f) {                // (the middle row of an odd h is its own mirror image)
                blk_a[e] = h - 1 - f;
                blk_b[e] = c + 1;
            }
        }
    }
    __syncthreads();

    int sweeps = 0, rotations = 0, converged = n < 2, g = 0, logged = 0, overflow = 0;
    const double tol2 = 1.1102230246251565e-16 * 1.1102230246251565e-16;      // (2^-53)^2
    for (int sweep = 0; sweep < kSpectralMaxSweeps && !converged && !overflow; ++sweep) {
        if (tid == 0) rotated[(sweep + 1) % 3] = 0;     // read last at the end of sweep - 2, counted in next
        for (int r = 0; r < m1; ++r, ++g) {
            // (1) one lane per pair: the rotation that annihilates a_pq, applied to its own 2 x 2 block
            if (tid == 0) round_active[(g + 1) & 1] = 0;
            if (tid < h) {
                int p, q;
                spectral_pair(r, tid, m1, p, q);
                const int ipp = spectral_at(p, p), iqq = spectral_at(q, q), ipq = spectral_at(p, q);
                const double app = A[ipp], aqq = A[iqq], apq = A[ipq];
                double c = 1.0, s = 0.0;
                if (apq * apq > tol2 * fabs(app * aqq)) {
                    // t = tan of the rotation angle, the smaller root of t^2 + 2 tau t - 1, tau = (aqq - app) / (2 apq):
                    // t = sign(tau) / (|tau| + sqrt(1 + tau^2)) = 2 apq sign(d) / (|d| + sqrt(d^2 + 4 apq^2)), d = aqq - app
                    // (entries of a Gram matrix of normalised basis columns: the squares stay far inside the normal range)
                    const double d = aqq - app, b2 = 2.0 * apq, w = d * d + b2 * b2;
                    const double t = (d >= 0.0 ? b2 : -b2) * spectral_rcp(fabs(d) + w * spectral_rsqrt(w));
                    c = spectral_rsqrt(1.0 + t * t);
                    s = t * c;
                    A[ipp] = app - t * apq;
                    A[iqq] = aqq + t * apq;
                    A[ipq] = 0.0;
                    atomicAdd(&rotated[sweep % 3], 1);
                    round_active[g & 1] = 1;
                }
                rot_c[tid] = c;
                rot_s[tid] = s;
            }
            __syncthreads();
            // uniform: nothing to rotate in this round.  (A lane may still be here while lane 0 clears this word for round
            // g + 2 -- only after a skipped round, when it holds 0 already.)
            if (!round_active[g & 1]) continue;
            if (logged >= a.log_rounds) {               // uniform
                overflow = 1;
                break;
            }
            if (tid < h) gstore2(a.d_log + (size_t)logged * h + tid, spectral_d2{rot_c[tid], rot_s[tid]});
            if (tid == 0) gstore_i(a.d_log_round + logged, r);
            ++logged;
            // (2) A <- J' A J off the pairs' own blocks
#pragma unroll
            for (int e = 0; e < kSpectralBlocksPerLane; ++e) {
                const int ka = blk_a[e], kb = blk_b[e];
                if (ka < 0) continue;
                int pa, qa, pb, qb;
                spectral_pair(r, ka, m1, pa, qa);
                spectral_pair(r, kb, m1, pb, qb);
                const int i00 = spectral_at(pa, pb), i01 = spectral_at(pa, qb), i10 = spectral_at(qa, pb), i11 = spectral_at(qa, qb);
                // (the rotations and the four numbers in one trip to LDS)
                const double ca = rot_c[ka], sa = rot_s[ka], cb = rot_c[kb], sb = rot_s[kb];
                const double x00 = A[i00], x01 = A[i01], x10 = A[i10], x11 = A[i11];
                if (sa == 0.0 && sb == 0.0) continue;
                // rows by J_a' ...
                const double r00 = ca * x00 - sa * x10, r01 = ca * x01 - sa * x11;
                const double r10 = sa * x00 + ca * x10, r11 = sa * x01 + ca * x11;
                // ... columns by J_b
                A[i00] = cb * r00 - sb * r01;
                A[i01] = sb * r00 + cb * r01;
                A[i10] = cb * r10 - sb * r11;
                A[i11] = sb * r10 + cb * r11;
            }
            __syncthreads();
        }
        if (overflow) break;
        const int done = rotated[sweep % 3];
        rotations += done;
        ++sweeps;
        converged = done == 0;
    }
    __syncthreads();
    if (tid < n) gstore(a.d_lam + tid, A[spectral_at(tid, tid)]);
    if (tid == 0) {
        a.d_hdr->logged = logged;
        a.d_hdr->sweeps = sweeps;
        a.d_hdr->rotations = rotations;
        a.d_hdr->converged = converged && !overflow;
    }
}

__device__ __forceinline__ double spectral_wave_sum(double x)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off, 64);
    return x;
}

__global__ __launch_bounds__(64 * kSpectralColumnsPerGroup) void spectral_vectors_kernel(const SpectralArgs *__restrict__ jobs)
{
    constexpr int W = kSpectralColumnsPerGroup, NMAX = kSpectralMaxColumns;
    __shared__ double col[W][NMAX + 2];
    __shared__ double lam_s[NMAX], xty_s[NMAX], ones_s[NMAX], qty_s[NMAX], bh_s[NMAX], sign_s[NMAX];
    __shared__ int order_s[NMAX];
    __shared__ double part_s[3 * NMAX][2];                  // double-double partial sums of the moments
    __shared__ int is_last;
    const SpectralArgs a = jobs[blockIdx.y];
    const int n = a.n, m = (n + 1) & ~1, h = m >> 1, m1 = m - 1;
    const int groups = (n + W - 1) / W;
    if ((int)blockIdx.x >= groups) return;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int column = blockIdx.x * W + wave;
    const SpectralHeader hdr = *a.d_hdr;

    // ---- replay the rotations on this wavefront's column of V' (starts as a unit vector).  The log comes through LDS in
    // chunks of kChunk rounds, the next chunk in flight (registers) while this one is applied: fetched round by round it
    // cost a trip to memory per round (0.8 of the 0.97 ms of a 66-column job).
    constexpr int kChunk = 16, kLoads = (kChunk * kSpectralMaxPairs + 64 * W - 1) / (64 * W);
    __shared__ spectral_d2 chunk_cs[kChunk * kSpectralMaxPairs];
    __shared__ int chunk_round[kChunk];
    double *v = col[wave];
    if (column < n)
        for (int j = lane; j < m; j += 64) v[j] = j == column ? 1.0 : 0.0;
    const int logged = hdr.logged;
    const bool two = h > 64;
    const int k0 = lane, k1 = lane + 64;
    spectral_d2 staged[kLoads];
    int staged_round = 0;
    auto fetch = [&](int first) {                           // rounds first .. first + kChunk - 1 -> registers
        const int rounds = min(kChunk, logged - first);
        const spectral_d2 *src = a.d_log + (size_t)first * h;
#pragma unroll
        for (int e = 0; e < kLoads; ++e) {
            const int at = tid + e * 64 * W;
            staged[e] = at < rounds * h ? gload2(src + at) : spectral_d2{1.0, 0.0};
        }
        staged_round = tid < rounds ? gload_i(a.d_log_round + first + tid) : 0;
    };
    if (logged > 0) fetch(0);
    for (int first = 0; first < logged; first += kChunk) {
        const int rounds = min(kChunk, logged - first);
        __syncthreads();                                    // the previous chunk has been applied by every wavefront
#pragma unroll
        for (int e = 0; e < kLoads; ++e) {
            const int at = tid + e * 64 * W;
            if (at < rounds * h) chunk_cs[at] = staged[e];
        }
        if (tid < rounds) chunk_round[tid] = staged_round;
        __syncthreads();
        if (first + kChunk < logged) fetch(first + kChunk);
        if (column < n) {
            for (int rr = 0; rr < rounds; ++rr) {
                const int r_now = chunk_round[rr];
                if (k0 < h) {
                    const spectral_d2 cs = chunk_cs[rr * h + k0];
                    if (cs.y != 0.0) {
                        int p, q;
                        spectral_pair(r_now, k0, m1, p, q);
                        const double vp = v[p], vq = v[q];
                        v[p] = cs.x * vp - cs.y * vq;
                        v[q] = cs.y * vp + cs.x * vq;
                    }
                }
                if (two && k1 < h) {
                    const spectral_d2 cs = chunk_cs[rr * h + k1];
                    if (cs.y != 0.0) {
                        int p, q;
                        spectral_pair(r_now, k1, m1, p, q);
                        const double vp = v[p], vq = v[q];
                        v[p] = cs.x * vp - cs.y * vq;
                        v[q] = cs.y * vp + cs.x * vq;
                    }
                }
            }
        }
    }
    if (column < n)
        for (int j = lane; j < n; j += 64) gstore(a.d_vt + (size_t)j * n + column, v[j]);

    // ---- the workgroup that completes the matrix finishes the job
    __threadfence();
    __syncthreads();
    if (tid == 0) is_last = atomicAdd(&a.d_hdr->arrived, 1) == groups - 1;
    __syncthreads();
    if (!is_last) return;
    __threadfence();                                        // (acquire: the other groups' columns)
    const int nthreads = blockDim.x, packed = (n * (n + 1)) >> 1;
    const double *in = a.in;
    for (int i = tid; i < n; i += nthreads) {
        lam_s[i] = gload(a.d_lam + i);
        xty_s[i] = gload(in + packed + i);
        ones_s[i] = gload(in + packed + n + i);
    }
    __syncthreads();
    // eigenvalues ascending (ties: by index)
    for (int i = tid; i < n; i += nthreads) {
        const double mine = lam_s[i];
        int rank = 0;
        for (int j = 0; j < n; ++j) {
            const double other = lam_s[j];
            rank += (other < mine || (other == mine && j < i)) ? 1 : 0;
        }
        order_s[rank] = i;
    }
    __syncthreads();
    double *out = a.out;
    double *o_lamb = out, *o_qty = out + n, *o_bh = out + 2 * n, *o_qt = out + 3 * n, *o_mom = out + 3 * n + (size_t)n * n;
    // eigenvector j = row order[j] of V': the sign convention (largest-magnitude component positive, the first one on
    // ties), Q'Xty, and the row itself to the result area -- one wavefront per vector
    for (int j = wave; j < n; j += W) {
        const double *row = a.d_vt + (size_t)order_s[j] * n;
        double x[(NMAX + 63) / 64];
        double best = -1.0;
        int piv = 0;
#pragma unroll
        for (int t = 0; t < (NMAX + 63) / 64; ++t) {
            const int i = lane + 64 * t;
            x[t] = i < n ? gload(row + i) : 0.0;
            if (i < n && fabs(x[t]) > best) {
                best = fabs(x[t]);
                piv = i;
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const double ob = __shfl_xor(best, off, 64);
            const int op = __shfl_xor(piv, off, 64);
            if (ob > best || (ob == best && op < piv)) {
                best = ob;
                piv = op;
            }
        }
        const double pivot = gload(row + piv);
        const double sign = (a.canonical && pivot < 0.0) ? -1.0 : 1.0;
        double acc = 0.0;
#pragma unroll
        for (int t = 0; t < (NMAX + 63) / 64; ++t) {
            const int i = lane + 64 * t;
            if (i < n) {
                const double val = sign * x[t];
                gstore(o_qt + (size_t)j * n + i, val);
                acc += val * xty_s[i];
            }
        }
        acc = spectral_wave_sum(acc);
        if (lane == 0) {
            sign_s[j] = sign;
            qty_s[j] = acc;
            gstore(o_lamb + j, lam_s[order_s[j]]);
            gstore(o_qty + j, acc);
        }
    }
    __syncthreads();
    // betahat = Q (qty / lamb)
    for (int i = tid; i < n; i += nthreads) {
        double acc = 0.0;
        for (int j = 0; j < n; ++j)
            acc += (sign_s[j] * gload(a.d_vt + (size_t)order_s[j] * n + i)) * (qty_s[j] / lam_s[order_s[j]]);
        bh_s[i] = acc;
        gstore(o_bh + i, acc);
    }
    __syncthreads();
    // residual moments of y - X betahat from the Gram alone: sum r = sum y - sum_j (1'x_j) b_j,
    // sum r^2 = y'y - 2 b'Xty + b'XtX b (cancels 3-4 digits: double-double, the entries of XtX as the caller gave them)
    dd *part = reinterpret_cast<dd *>(&part_s[0][0]);
    for (int i = tid; i < n; i += nthreads) {
        dd acc = {0.0, 0.0};
        for (int j = 0; j < n; ++j) acc = dd_add(acc, dd_prod(gload(a.d_a + spectral_at(i, j)), bh_s[j]));
        part[3 * i + 0] = dd_mul_d(acc, bh_s[i]);
        part[3 * i + 1] = dd_prod(xty_s[i], bh_s[i]);
        part[3 * i + 2] = dd_prod(ones_s[i], bh_s[i]);
    }
    __syncthreads();
    if (tid == 0) {
        dd quad = {0.0, 0.0}, cross = {0.0, 0.0}, s1 = {gload(in + packed + 2 * n), 0.0};
        for (int i = 0; i < n; ++i) {
            quad = dd_add(quad, part[3 * i + 0]);
            cross = dd_add(cross, part[3 * i + 1]);
            s1 = dd_add(s1, {-part[3 * i + 2].hi, -part[3 * i + 2].lo});
        }
        const dd yty = {gload(in + packed + 2 * n + 1), 0.0};
        const dd ssr = dd_add(dd_add(yty, {-2.0 * cross.hi, -2.0 * cross.lo}), quad);
        gstore(o_mom + 0, s1.hi + s1.lo);
        gstore(o_mom + 1, ssr.hi + ssr.lo);
        gstore(o_mom + 2, (double)hdr.sweeps);
        gstore(o_mom + 3, (double)hdr.rotations);
        gstore(o_mom + 4, (double)(wall_clock64() - hdr.t_begin) * a.seconds_per_tick);
        gstore(o_mom + 5, hdr.converged ? 0.0 : 1.0);
    }
    // every wavefront has stored rows of Q', eigenvalues and betahat into the result area (fokl_chain_device.inc: the order)
    publish_ticket(o_mom + 6, a.ticket);
}

}  // namespace fokl

namespace {

constexpr int kSpectralStreams = 4;
constexpr int kSpectralRing = 8192;                         // argument records in rotation (page-locked)
constexpr int kSpectralClasses = 3;                         // result areas by size: up to 48, 96, all columns
constexpr int kSpectralClassColumns[kSpectralClasses] = {48, 96, fokl::kSpectralMaxColumns};
constexpr int kSpectralSlabSlots[kSpectralClasses] = {128, 128, 32};
constexpr int kSpectralWorkAreas = 64;                      // jobs in flight on the device at most

inline size_t spectral_in_doubles(int n) { return (size_t)n * (n + 1) / 2 + 2 * (size_t)n + 2; }
inline size_t spectral_out_doubles(int n) { return (size_t)n * n + 3 * (size_t)n + 7; }

struct SpectralWork {                                       // device memory for one job in flight
    double *d_a = nullptr, *d_vt = nullptr, *d_lam = nullptr;
    spectral_d2 *d_log = nullptr;
    int *d_log_round = nullptr;
    fokl::SpectralHeader *d_hdr = nullptr;
    int log_rounds = 0;
};

struct SpectralSlot {
    double *in = nullptr, *out = nullptr;                   // page-locked, room for the slot's class
    int cls = 0;
    int64_t ticket = 0;                                     // 0: free
    int n = 0;
    int stream = -1;                                        // -1: staged, not launched yet
    SpectralWork *work = nullptr;                           // while in flight
};

}  // namespace

struct fokl_dspectral {
    int device = 0;
    hipStream_t streams[kSpectralStreams] = {};
    int next_stream = 0;
    double seconds_per_tick = 1e-8;
    std::mutex m;
    std::vector<char *> slabs;
    std::vector<SpectralSlot *> slots, free_slots[kSpectralClasses];
    std::map<int64_t, SpectralSlot *> jobs;                 // every job not released yet
    std::vector<SpectralSlot *> pending;                    // staged since the last launch
    std::deque<SpectralSlot *> inflight;                    // launched, completion not seen yet (oldest first)
    std::vector<SpectralWork *> works, free_works;
    char *work_slab = nullptr;
    fokl::SpectralArgs *ring = nullptr;                     // page-locked
    size_t ring_at = 0;
    int64_t next_ticket = 1;
    bool canonical = true;
    std::atomic<int64_t> submitted{0}, launches{0};
    std::string err;
};

namespace {

int dspectral_fail(fokl_dspectral *e, int code, const std::string &msg)
{
    if (e) e->err = msg;
    fokl_set_global_error(msg);
    return code;
}

#define DSPECTRAL_TRY(e, call)                                                                                 \
    do {                                                                                                       \
        hipError_t e__ = (call);                                                                               \
        if (e__ != hipSuccess)                                                                                 \
            return dspectral_fail(e, FOKL_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e__));        \
    } while (0)

inline const double *spectral_flag(const SpectralSlot *s) { return s->out + 3 * (size_t)s->n + (size_t)s->n * s->n + 6; }

inline bool spectral_has_run(const SpectralSlot *s)
{
    double seen;
    __atomic_load(spectral_flag(s), &seen, __ATOMIC_ACQUIRE);
    return seen == (double)s->ticket;
}

inline int spectral_class(int n)
{
    for (int c = 0; c < kSpectralClasses; ++c)
        if (n <= kSpectralClassColumns[c]) return c;
    return kSpectralClasses - 1;
}

int spectral_more_slots(fokl_dspectral *e, int cls)
{
    const int cols = kSpectralClassColumns[cls];
    const size_t per_slot = (spectral_in_doubles(cols) + spectral_out_doubles(cols) + 15) / 8 * 8;
    char *slab = nullptr;
    DSPECTRAL_TRY(e, hipHostMalloc((void **)&slab, per_slot * sizeof(double) * kSpectralSlabSlots[cls], hipHostMallocDefault));
    e->slabs.push_back(slab);
    for (int i = 0; i < kSpectralSlabSlots[cls]; ++i) {
        auto *s = new SpectralSlot();
        s->in = reinterpret_cast<double *>(slab) + (size_t)i * per_slot;
        s->out = s->in + spectral_in_doubles(cols);
        s->cls = cls;
        e->slots.push_back(s);
        e->free_slots[cls].push_back(s);
    }
    return FOKL_OK;
}

int spectral_make_works(fokl_dspectral *e)
{
    const size_t nmax = fokl::kSpectralMaxColumns, hmax = fokl::kSpectralMaxPairs;
    const size_t log_rounds = (size_t)fokl::kSpectralLogSweeps * (nmax - 1);
    auto up = [](size_t b) { return (b + 255) / 256 * 256; };
    const size_t b_a = up(nmax * nmax * 8), b_lam = up(nmax * 8), b_log = up(log_rounds * hmax * sizeof(spectral_d2)),
                 b_round = up(log_rounds * sizeof(int)), b_hdr = up(sizeof(fokl::SpectralHeader));
    const size_t per = 2 * b_a + b_lam + b_log + b_round + b_hdr;
    DSPECTRAL_TRY(e, hipMalloc((void **)&e->work_slab, per * kSpectralWorkAreas));
    DSPECTRAL_TRY(e, hipMemset(e->work_slab, 0, per * kSpectralWorkAreas));
    for (int i = 0; i < kSpectralWorkAreas; ++i) {
        auto *w = new SpectralWork();
        char *at = e->work_slab + (size_t)i * per;
        w->d_a = reinterpret_cast<double *>(at);
        at += b_a;
        w->d_vt = reinterpret_cast<double *>(at);
        at += b_a;
        w->d_lam = reinterpret_cast<double *>(at);
        at += b_lam;
        w->d_log = reinterpret_cast<spectral_d2 *>(at);
        at += b_log;
        w->d_log_round = reinterpret_cast<int *>(at);
        at += b_round;
        w->d_hdr = reinterpret_cast<fokl::SpectralHeader *>(at);
        w->log_rounds = (int)log_rounds;
        e->works.push_back(w);
        e->free_works.push_back(w);
    }
    return FOKL_OK;
}

// Work areas of jobs that have run go back to the pool (caller holds e->m).
void spectral_reap(fokl_dspectral *e)
{
    for (auto it = e->inflight.begin(); it != e->inflight.end();) {
        SpectralSlot *s = *it;
        if (spectral_has_run(s)) {
            e->free_works.push_back(s->work);
            s->work = nullptr;
            it = e->inflight.erase(it);
        } else {
            ++it;
        }
    }
}

// enough lanes for one off-diagonal block each where that is possible (h (h - 1) / 2 blocks, folded to ceil(h / 2) (h - 1))
inline int spectral_threads(int n)
{
    const int h = (n + 1) / 2, blocks = ((h + 1) / 2) * std::max(h - 1, 1);
    return blocks <= 256 ? 256 : (blocks <= 512 ? 512 : 1024);
}
inline size_t spectral_lds_bytes(int n)
{
    const size_t m = (size_t)((n + 1) & ~1);
    return (m * (m + 1) / 2) * sizeof(double);
}

// Launch what is staged (caller holds e->m): the jobs of one launch share the block size of the largest of them and the
// dynamic LDS it needs.  A job needs a work area: when all are in flight, the oldest jobs are waited for.
int spectral_launch(fokl_dspectral *e)
{
    size_t at = 0;
    while (at < e->pending.size()) {
        if (e->ring_at >= (size_t)kSpectralRing) e->ring_at = 0;
        spectral_reap(e);
        for (int spins = 0; e->free_works.empty(); ++spins) {
            if (spins > 400000) return dspectral_fail(e, FOKL_ERR_STATE, "device spectral: jobs in flight never ran");
            std::this_thread::sleep_for(std::chrono::microseconds(10));
            spectral_reap(e);
        }
        const size_t count = std::min(std::min(e->pending.size() - at, (size_t)kSpectralRing - e->ring_at), e->free_works.size());
        int n_max = 1;
        for (size_t k = 0; k < count; ++k) {
            SpectralSlot *s = e->pending[at + k];
            SpectralWork *w = e->free_works.back();
            e->free_works.pop_back();
            s->work = w;
            fokl::SpectralArgs &args = e->ring[e->ring_at + k];
            args.in = s->in;
            args.out = s->out;
            args.d_a = w->d_a;
            args.d_vt = w->d_vt;
            args.d_lam = w->d_lam;
            args.d_log = w->d_log;
            args.d_log_round = w->d_log_round;
            args.d_hdr = w->d_hdr;
            args.ticket = (double)s->ticket;
            args.seconds_per_tick = e->seconds_per_tick;
            args.n = s->n;
            args.canonical = e->canonical ? 1 : 0;
            args.log_rounds = w->log_rounds;
            n_max = std::max(n_max, s->n);
            s->stream = e->next_stream;
            e->inflight.push_back(s);
        }
        hipStream_t stream = e->streams[e->next_stream];
        e->next_stream = (e->next_stream + 1) % kSpectralStreams;
        const fokl::SpectralArgs *d_args = e->ring + e->ring_at;
        hipLaunchKernelGGL(fokl::spectral_sweep_kernel, dim3((unsigned)count), dim3((unsigned)spectral_threads(n_max)),
                           spectral_lds_bytes(n_max), stream, d_args);
        const unsigned groups = (unsigned)((n_max + fokl::kSpectralColumnsPerGroup - 1) / fokl::kSpectralColumnsPerGroup);
        hipLaunchKernelGGL(fokl::spectral_vectors_kernel, dim3(groups, (unsigned)count),
                           dim3(64 * fokl::kSpectralColumnsPerGroup), 0, stream, d_args);
        DSPECTRAL_TRY(e, hipGetLastError());
        e->launches.fetch_add(1, std::memory_order_relaxed);
        e->ring_at += count;
        at += count;
    }
    e->pending.clear();
    return FOKL_OK;
}

}  // namespace

extern "C" int fokl_dspectral_create(int device, fokl_dspectral **out)
{
    if (!out) return dspectral_fail(nullptr, FOKL_ERR_ARG, "fokl_dspectral_create: null pointer");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count)
        return dspectral_fail(nullptr, FOKL_ERR_HIP, "fokl_dspectral_create: no such HIP device");
    if (hipSetDevice(device) != hipSuccess) return dspectral_fail(nullptr, FOKL_ERR_HIP, "fokl_dspectral_create: hipSetDevice failed");
    auto *e = new fokl_dspectral();
    e->device = device;
    for (int i = 0; i < kSpectralStreams; ++i)
        if (hipStreamCreateWithFlags(&e->streams[i], hipStreamNonBlocking) != hipSuccess) {
            for (int j = 0; j < i; ++j) (void)hipStreamDestroy(e->streams[j]);
            delete e;
            return dspectral_fail(nullptr, FOKL_ERR_HIP, "fokl_dspectral_create: hipStreamCreate failed");
        }
    int khz = 0;
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device) == hipSuccess && khz > 0)
        e->seconds_per_tick = 1e-3 / (double)khz;
    hipError_t rc = hipFuncSetAttribute(reinterpret_cast<const void *>(fokl::spectral_sweep_kernel),
                                        hipFuncAttributeMaxDynamicSharedMemorySize,
                                        (int)spectral_lds_bytes(fokl::kSpectralMaxColumns));
    if (rc == hipSuccess) rc = hipHostMalloc((void **)&e->ring, sizeof(fokl::SpectralArgs) * kSpectralRing, hipHostMallocDefault);
    if (rc != hipSuccess || spectral_make_works(e) != FOKL_OK) {
        const std::string why = rc != hipSuccess ? hipGetErrorString(rc) : e->err;
        fokl_dspectral_destroy(e);
        return dspectral_fail(nullptr, FOKL_ERR_HIP, "fokl_dspectral_create: " + why);
    }
    *out = e;
    return FOKL_OK;
}

extern "C" void fokl_dspectral_destroy(fokl_dspectral *e)
{
    if (!e) return;
    (void)hipSetDevice(e->device);
    for (auto &st : e->streams)
        if (st) (void)hipStreamSynchronize(st);
    for (auto *s : e->slots) delete s;
    for (auto *w : e->works) delete w;
    for (char *slab : e->slabs) (void)hipHostFree(slab);
    if (e->work_slab) (void)hipFree(e->work_slab);
    if (e->ring) (void)hipHostFree(e->ring);
    for (auto &st : e->streams)
        if (st) (void)hipStreamDestroy(st);
    delete e;
}

extern "C" int fokl_dspectral_max_columns(void) { return fokl::kSpectralMaxColumns; }

extern "C" int fokl_dspectral_set_signs(fokl_dspectral *e, int canonical)
{
    if (!e) return dspectral_fail(nullptr, FOKL_ERR_ARG, "fokl_dspectral_set_signs: null engine");
    std::lock_guard<std::mutex> lock(e->m);
    e->canonical = canonical != 0;
    return FOKL_OK;
}

extern "C" int fokl_dspectral_submit(fokl_dspectral *e, const double *gram, int ld, const int32_t *idx, int p1, int ycol,
                                     int launch, int64_t *ticket, double **result)
{
    if (!e || !gram || !idx || !ticket || !result || p1 < 1 || p1 > fokl::kSpectralMaxColumns || ld < 1 || ycol < 0 ||
        ycol >= ld)
        return dspectral_fail(e, FOKL_ERR_ARG, "fokl_dspectral_submit: null pointer, empty or too large a model, or y column out of range");
    for (int i = 0; i < p1; ++i)
        if (idx[i] < 0 || idx[i] >= ld) return dspectral_fail(e, FOKL_ERR_ARG, "fokl_dspectral_submit: column index out of range");
    std::lock_guard<std::mutex> lock(e->m);
    const int cls = spectral_class(p1);
    if (e->free_slots[cls].empty()) {
        (void)hipSetDevice(e->device);
        const int rc = spectral_more_slots(e, cls);
        if (rc) return rc;
    }
    SpectralSlot *s = e->free_slots[cls].back();
    e->free_slots[cls].pop_back();
    s->ticket = e->next_ticket++;
    s->n = p1;
    s->stream = -1;
    s->work = nullptr;
    // the sub-block (its lower triangle is what the kernel reads: LAPACK's uplo = 'L'), Xty, the ones row, two scalars
    double *a = s->in, *xty = a + (size_t)p1 * (p1 + 1) / 2, *ones = xty + p1;
    const size_t ldz = (size_t)ld;
    for (int i = 0; i < p1; ++i) {
        const double *row = gram + (size_t)idx[i] * ldz;
        double *packed_row = a + (size_t)i * (i + 1) / 2;
        for (int j = 0; j <= i; ++j) packed_row[j] = row[idx[j]];
        xty[i] = row[ycol];
        ones[i] = gram[idx[i]];
    }
    ones[p1] = gram[ycol];
    ones[p1 + 1] = gram[(size_t)ycol * ldz + ycol];
    double reset = 0.0;
    __atomic_store(const_cast<double *>(spectral_flag(s)), &reset, __ATOMIC_RELEASE);
    e->jobs[s->ticket] = s;
    e->pending.push_back(s);
    e->submitted.fetch_add(1, std::memory_order_relaxed);
    *ticket = s->ticket;
    *result = s->out;
    if (launch) {
        (void)hipSetDevice(e->device);
        return spectral_launch(e);
    }
    return FOKL_OK;
}

extern "C" int fokl_dspectral_flush(fokl_dspectral *e)
{
    if (!e) return dspectral_fail(nullptr, FOKL_ERR_ARG, "fokl_dspectral_flush: null engine");
    std::lock_guard<std::mutex> lock(e->m);
    if (e->pending.empty()) return FOKL_OK;
    (void)hipSetDevice(e->device);
    return spectral_launch(e);
}

// 1 = the job has run, 0 = not yet, < 0 = error
extern "C" int fokl_dspectral_poll(fokl_dspectral *e, int64_t ticket)
{
    if (!e) return -dspectral_fail(nullptr, FOKL_ERR_ARG, "fokl_dspectral_poll: null engine");
    SpectralSlot *s = nullptr;
    {
        std::lock_guard<std::mutex> lock(e->m);
        auto it = e->jobs.find(ticket);
        if (it == e->jobs.end()) return -dspectral_fail(e, FOKL_ERR_ARG, "device spectral: unknown or released ticket");
        s = it->second;
        if (s->stream < 0) {
            (void)hipSetDevice(e->device);
            const int rc = spectral_launch(e);
            if (rc) return -rc;
        }
    }
    return spectral_has_run(s) ? 1 : 0;
}

extern "C" int fokl_dspectral_wait(fokl_dspectral *e, int64_t ticket)
{
    if (!e) return dspectral_fail(nullptr, FOKL_ERR_ARG, "fokl_dspectral_wait: null engine");
    SpectralSlot *s = nullptr;
    hipStream_t stream = nullptr;
    {
        std::lock_guard<std::mutex> lock(e->m);
        auto it = e->jobs.find(ticket);
        if (it == e->jobs.end()) return dspectral_fail(e, FOKL_ERR_ARG, "device spectral: unknown or released ticket");
        s = it->second;
        if (s->stream < 0) {
            (void)hipSetDevice(e->device);
            const int rc = spectral_launch(e);
            if (rc) return rc;
        }
        stream = e->streams[s->stream];
    }
    for (int spins = 0; !spectral_has_run(s); ++spins) {
        if (spins >= 2000 && spins % 500 == 0) {
            const hipError_t st = hipStreamQuery(stream);
            if (st != hipErrorNotReady) {
                if (spectral_has_run(s)) break;
                return dspectral_fail(e, FOKL_ERR_HIP, "device spectral: the kernels never stored the job's ticket");
            }
        }
        if (spins < 2000) {
            __builtin_ia32_pause();
        } else {
            std::this_thread::sleep_for(std::chrono::microseconds(20));
        }
    }
    const double not_converged = s->out[3 * (size_t)s->n + (size_t)s->n * s->n + 5];
    if (not_converged != 0.0) return dspectral_fail(e, FOKL_ERR_NUMERIC, "device spectral: Jacobi sweeps did not converge");
    return FOKL_OK;
}

// Frees the job's result area (after the kernels have run: a job that is still in flight is waited for).  Idempotent.
extern "C" int fokl_dspectral_release(fokl_dspectral *e, int64_t ticket)
{
    if (!e) return dspectral_fail(nullptr, FOKL_ERR_ARG, "fokl_dspectral_release: null engine");
    {
        std::lock_guard<std::mutex> lock(e->m);
        if (e->jobs.find(ticket) == e->jobs.end()) return FOKL_OK;
    }
    const int rc = fokl_dspectral_wait(e, ticket);
    std::lock_guard<std::mutex> lock(e->m);
    auto it = e->jobs.find(ticket);
    if (it == e->jobs.end()) return FOKL_OK;
    SpectralSlot *s = it->second;
    e->jobs.erase(it);
    if (s->work) {                                          // in flight until now: its work area goes back with it
        for (auto f = e->inflight.begin(); f != e->inflight.end(); ++f)
            if (*f == s) {
                e->inflight.erase(f);
                break;
            }
        if (rc == FOKL_OK || rc == FOKL_ERR_NUMERIC) e->free_works.push_back(s->work);   // (else the device may still write it)
        s->work = nullptr;
    }
    s->ticket = 0;
    e->free_slots[s->cls].push_back(s);
    return rc == FOKL_ERR_NUMERIC ? FOKL_OK : rc;
}

extern "C" int fokl_dspectral_stats(fokl_dspectral *e, int64_t *submitted, int64_t *launches)
{
    if (!e) return dspectral_fail(nullptr, FOKL_ERR_ARG, "fokl_dspectral_stats: null engine");
    if (submitted) *submitted = e->submitted.load(std::memory_order_relaxed);
    if (launches) *launches = e->launches.load(std::memory_order_relaxed);
    return FOKL_OK;
}

// The Gibbs recursion of a host chain with its PIECES ACROSS SIMD LANES (fokl_gibbs_chain_segments_host in fokl_sampler.cpp
// cuts the chain and checks the cuts; this file is one step loop over up to eight pieces at once).
//
// Included three times -- fokl_sampler.cpp (portable), fokl_vlog.cpp (AVX2), fokl_sampler.cpp built as the AVX-512 recorder
// -- with FOKL_CHAIN_LANES_NAME naming the function.  One source for all three: arithmetic is written on GCC's generic
// vectors of eight doubles (lane = piece), which each build lowers to what it has (one zmm, two ymm, four xmm); only
// the 8 x 8 transposes between the tape's [row][column] layout and [column][piece] registers are written per ISA, and
// they move data without touching it.
//
// Within a piece an iteration is chain_step of fokl_sampler.cpp: the same per-element expressions, IEEE add / mul / div /
// sqrt, no contraction (-ffp-contract=off), and the three sums with element i in partial sum i mod 8, combined in the
// order of chain_vector_portable.  A piece's rows therefore are bit for bit what the serial recursion produces from the
// same entering state, in every build.
#include <cstdint>

#pragma GCC diagnostic ignored "-Wpsabi"      // 64-byte vectors by value between functions local to the including file

#ifndef FOKL_CHAIN_LANES_TYPES
#define FOKL_CHAIN_LANES_TYPES
constexpr int kLanePieces = 8;

// what does not change from step to step
struct fokl_lane_chain {
    const double *lamb, *qty, *normals, *gam_sig, *gam_tau;
    double *w_out, *sigs_out, *taus_out;                    // rows / entries before a piece's first own iteration stay unwritten
    int p1, draws, pieces, piece, warm;
    double b, btau, dtd;
};

// piece s runs iterations [max(s piece - warm, 0), min((s + 1) piece, draws)); at step j it is at s piece - warm + j
struct fokl_lane_state {
    double sigsqd[kLanePieces], tausqd[kLanePieces];        // the state each piece holds now
    double begin[kLanePieces][2];                           // ... and held in front of its first own iteration s piece
    int32_t flagged;                                        // bstar < 0 met in any piece, warm-up included
};
#endif

namespace {

typedef double lane_v8 __attribute__((vector_size(64)));
typedef long long lane_m8 __attribute__((vector_size(64)));

#if defined(__AVX512F__)
inline lane_v8 lane_sqrt(lane_v8 x) { return (lane_v8)_mm512_sqrt_pd((__m512d)x); }

// r[l] = eight consecutive doubles of row l  ->  r[c] = element c of the eight rows (and back: the map is its own inverse)
inline void lane_transpose(lane_v8 (&r)[8])
{
    const __m512d t0 = _mm512_unpacklo_pd((__m512d)r[0], (__m512d)r[1]), t1 = _mm512_unpackhi_pd((__m512d)r[0], (__m512d)r[1]);
    const __m512d t2 = _mm512_unpacklo_pd((__m512d)r[2], (__m512d)r[3]), t3 = _mm512_unpackhi_pd((__m512d)r[2], (__m512d)r[3]);
    const __m512d t4 = _mm512_unpacklo_pd((__m512d)r[4], (__m512d)r[5]), t5 = _mm512_unpackhi_pd((__m512d)r[4], (__m512d)r[5]);
    const __m512d t6 = _mm512_unpacklo_pd((__m512d)r[6], (__m512d)r[7]), t7 = _mm512_unpackhi_pd((__m512d)r[6], (__m512d)r[7]);
    const __m512d u0 = _mm512_shuffle_f64x2(t0, t2, 0x88), u1 = _mm512_shuffle_f64x2(t0, t2, 0xdd);
    const __m512d u2 = _mm512_shuffle_f64x2(t4, t6, 0x88), u3 = _mm512_shuffle_f64x2(t4, t6, 0xdd);
    const __m512d u4 = _mm512_shuffle_f64x2(t1, t3, 0x88), u5 = _mm512_shuffle_f64x2(t1, t3, 0xdd);
    const __m512d u6 = _mm512_shuffle_f64x2(t5, t7, 0x88), u7 = _mm512_shuffle_f64x2(t5, t7, 0xdd);
    r[0] = (lane_v8)_mm512_shuffle_f64x2(u0, u2, 0x88);
    r[4] = (lane_v8)_mm512_shuffle_f64x2(u0, u2, 0xdd);
    r[2] = (lane_v8)_mm512_shuffle_f64x2(u1, u3, 0x88);
    r[6] = (lane_v8)_mm512_shuffle_f64x2(u1, u3, 0xdd);
    r[1] = (lane_v8)_mm512_shuffle_f64x2(u4, u6, 0x88);
    r[5] = (lane_v8)_mm512_shuffle_f64x2(u4, u6, 0xdd);
    r[3] = (lane_v8)_mm512_shuffle_f64x2(u5, u7, 0x88);
    r[7] = (lane_v8)_mm512_shuffle_f64x2(u5, u7, 0xdd);
}
#else
inline lane_v8 lane_sqrt(lane_v8 x)
{
    lane_v8 r;
#if defined(__AVX2__)
    double in[8], out[8];
    __builtin_memcpy(in, &x, sizeof in);
    _mm256_storeu_pd(out, _mm256_sqrt_pd(_mm256_loadu_pd(in)));
    _mm256_storeu_pd(out + 4, _mm256_sqrt_pd(_mm256_loadu_pd(in + 4)));
    __builtin_memcpy(&r, out, sizeof out);
#else
    for (int l = 0; l < 8; ++l) r[l] = __builtin_sqrt(x[l]);
#endif
    return r;
}

inline void lane_transpose(lane_v8 (&r)[8])
{
    double a[8][8];
    __builtin_memcpy(a, r, sizeof a);
    for (int c = 0; c < 8; ++c)
        for (int l = 0; l < 8; ++l) r[c][l] = a[l][c];
}
#endif

#if defined(__AVX512F__)
inline lane_v8 lane_load(const double *p) { return (lane_v8)_mm512_loadu_pd(p); }
inline void lane_store(double *p, lane_v8 v) { _mm512_storeu_pd(p, (__m512d)v); }
#else
inline lane_v8 lane_load(const double *p)
{
    lane_v8 v;
    __builtin_memcpy(&v, p, sizeof v);
    return v;
}

inline void lane_store(double *p, lane_v8 v) { __builtin_memcpy(p, &v, sizeof v); }
#endif

// the eight partial sums of one quadratic form, in chain_vector_portable's order
inline lane_v8 lane_combine(const lane_v8 (&a)[8])
{
    return ((a[0] + a[4]) + (a[2] + a[6])) + ((a[1] + a[5]) + (a[3] + a[7]));
}

}  // namespace

// steps [j0, j1) of all pieces; the caller has made sure the tape's rows they read are complete
extern "C" __attribute__((visibility("hidden"))) void FOKL_CHAIN_LANES_NAME(const fokl_lane_chain *chain,
                                                                            fokl_lane_state *state, int j0, int j1)
{
    const fokl_lane_chain &c = *chain;
    const int p1 = c.p1, draws = c.draws, full = p1 & ~7;
    const size_t ahead = (size_t)(4 * p1 > 512 ? 4 * p1 : 512);         // doubles: four rows, 4 KB at least
    lane_v8 sigsqd = lane_load(state->sigsqd), tausqd = lane_load(state->tausqd);
    int k_write[8], k_end[8];
    for (int s = 0; s < 8; ++s) {
        k_write[s] = s * c.piece < draws ? s * c.piece : draws;
        k_end[s] = s < c.pieces ? (k_write[s] + c.piece < draws ? k_write[s] + c.piece : draws) : k_write[s];
    }
    for (int j = j0; j < j1; ++j) {
        const double *row[8];
        double *out[8];
        lane_m8 active;
        lane_v8 gs, gt;
        bool real[8], all_real = true;
        for (int s = 0; s < 8; ++s) {
            const int k = s * c.piece - c.warm + j;
            const bool on = k >= 0 && k < k_end[s];
            const int kc = k < 0 ? 0 : (k < draws ? k : draws - 1);
            active[s] = on ? -1 : 0;
            real[s] = on && k >= k_write[s];
            all_real = all_real && real[s];
            row[s] = c.normals + (size_t)kc * p1;
            out[s] = c.w_out + (size_t)kc * p1;
            gs[s] = c.gam_sig[kc];
            gt[s] = c.gam_tau[kc];
            if (on && k == k_write[s]) {
                state->begin[s][0] = sigsqd[s];
                state->begin[s][1] = tausqd[s];
            }
        }
        const lane_v8 inv_tau = 1.0 / tausqd, sig = lane_sqrt(sigsqd);
        lane_v8 a_lam[8], a_ty[8], a_ww[8];
#pragma GCC unroll 8
        for (int l = 0; l < 8; ++l) a_lam[l] = a_ty[l] = a_ww[l] = lane_v8{0, 0, 0, 0, 0, 0, 0, 0};
        int i0 = 0;
        for (; i0 < full; i0 += 8) {
            lane_v8 v[8];
            for (int s = 0; s < 8; ++s) {
                // (eight slow streams through a tape other cores have written: the hardware prefetchers follow one fast
                // stream better than these)
                __builtin_prefetch(row[s] + i0 + ahead);
                v[s] = lane_load(row[s] + i0);
            }
            lane_transpose(v);
#pragma GCC unroll 8
            for (int l = 0; l < 8; ++l) {
                const double la = c.lamb[i0 + l], q = c.qty[i0 + l];
                const lane_v8 d = 1.0 / (la + inv_tau);
                const lane_v8 wi = d * q + sig * (lane_sqrt(d) * v[l]);
                v[l] = wi;
                const lane_v8 ww = wi * wi;
                a_lam[l] += la * ww;
                a_ty[l] += wi * q;
                a_ww[l] += ww;
            }
            lane_transpose(v);
            if (all_real) {
                for (int s = 0; s < 8; ++s) lane_store(out[s] + i0, v[s]);
            } else {
                for (int s = 0; s < 8; ++s)
                    if (real[s]) lane_store(out[s] + i0, v[s]);
            }
        }
        // the columns beyond the last full eight: partial sums 0 .. (indices the compiler can see: the sums stay in registers)
#pragma GCC unroll 8
        for (int l = 0; l < 7; ++l) {
            const int i = i0 + l;
            if (i >= p1) break;
            lane_v8 vi;
            for (int s = 0; s < 8; ++s) vi[s] = row[s][i];
            const double la = c.lamb[i], q = c.qty[i];
            const lane_v8 d = 1.0 / (la + inv_tau);
            const lane_v8 wi = d * q + sig * (lane_sqrt(d) * vi);
            for (int s = 0; s < 8; ++s)
                if (real[s]) out[s][i] = wi[s];
            const lane_v8 ww = wi * wi;
            a_lam[l] += la * ww;
            a_ty[l] += wi * q;
            a_ww[l] += ww;
        }
        // chain_step's scalar half, all pieces at once
        const lane_v8 q_lam = lane_combine(a_lam), q_ty = lane_combine(a_ty), q_ww = lane_combine(a_ww);
        const lane_v8 bstar = c.b + 0.5 * (q_lam - 2.0 * q_ty + c.dtd + q_ww / tausqd);
        const lane_m8 negative = bstar < 0.0;
        const lane_v8 nan = lane_v8{0, 0, 0, 0, 0, 0, 0, 0} + __builtin_nan("");
        const lane_v8 sig_next = negative ? nan : 1.0 / ((1.0 / bstar) * gs);
        const lane_v8 btau_star = (1.0 / (2.0 * sig_next)) * q_ww + c.btau;
        const lane_v8 tau_next = 1.0 / ((1.0 / btau_star) * gt);
        const lane_m8 hit = negative & active;
        for (int s = 0; s < 8; ++s)
            if (hit[s]) state->flagged = 1;
        sigsqd = active ? sig_next : sigsqd;
        tausqd = active ? tau_next : tausqd;
        for (int s = 0; s < 8; ++s) {
            if (!real[s]) continue;
            const int k = s * c.piece - c.warm + j;
            if (c.sigs_out) c.sigs_out[k] = sigsqd[s];
            if (c.taus_out) c.taus_out[k] = tausqd[s];
        }
    }
    lane_store(state->sigsqd, sigsqd);
    lane_store(state->tausqd, tausqd);
}

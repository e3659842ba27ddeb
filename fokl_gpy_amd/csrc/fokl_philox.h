// The random numbers of the embedded-GP sampler (fokl_embedded_device.inc, fokl_embedded.cpp) and of the posterior
// resampler (fokl_resample_device.inc): Philox 4x32-10, counter based, so the kernel and the host statement draw the same
// numbers without sharing a state.  One header for both sides.
//
//   key     = (seed, chain)                  counter = (draw, purpose, index, 0)
//   words   = philox4x32_10(counter, key)    -> two uniforms of 53 bits, u_a from words 0-1 and u_b from words 2-3
//   uniform = u_a                            in [0, 1)
//   normal  = sqrt(-2 ln(1 - u_a)) cos(2 pi u_b)          (Box-Muller, one normal per counter: 1 - u_a is in (0, 1])
//
// The ensemble sampler over unknown inputs (fokl_infer_device.inc) draws from streams of its own: the same key and counter
// layout with the fourth counter word 1 (inf_uniform, inf_normal below).
//
// The particle filter over a fitted dynamic system (fokl_assimilate_device.inc) draws from a third family: the same key and
// counter layout with the fourth counter word 2 (asm_uniform, asm_normal below).
//
// The calibration of a fitted dynamic system (fokl_calibrate_device.inc) draws from a fourth family: the same key and
// counter layout with the fourth counter word 3 (cal_uniform, cal_normal below).
//
// The robust resampler (fokl_robust_device.inc, robust.py) draws from a fifth family: key (seed, chain), counter (iteration,
// purpose + 16 attempt, index, 4) (rob_uniform, rob_normal below): the attempt of a Marsaglia-Tsang variate rides in the
// purpose word, so that the index is free to name the row.
//
// Nothing here touches numpy's global stream or the fit's MT19937 machinery.
#ifndef FOKL_PHILOX_H
#define FOKL_PHILOX_H

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define FOKL_HD __host__ __device__ inline
#else
#define FOKL_HD inline
#endif

namespace fokl {

constexpr int EMB_PURPOSE_MOMENTUM = 0;   // the momentum of transition `draw`
constexpr int EMB_PURPOSE_ACCEPT = 1;     // its accept uniform (index 0)
constexpr int EMB_PURPOSE_SEARCH = 2;     // the momentum of the step search that runs at `draw` (0, or the mass update's)
// fokl_resample_device.inc / resample.py: `draw` is the Gibbs iteration (burn-in included)
constexpr int RES_PURPOSE_BETA = 3;       // the normal of eigen-coordinate `index`
constexpr int RES_PURPOSE_SIG_NORMAL = 4; // sigma^2's gamma: the normal of Marsaglia-Tsang attempt `index` ...
constexpr int RES_PURPOSE_SIG_UNIFORM = 5;   // ... and its uniform
constexpr int RES_PURPOSE_TAU_NORMAL = 6; // tau^2's gamma: the same two
constexpr int RES_PURPOSE_TAU_UNIFORM = 7;
constexpr int RES_PURPOSE_START = 8;      // draw 0: the uniforms behind a dispersed start (index 0 sigma^2, 1 tau^2)
constexpr int EMB_PURPOSE_LAST = RES_PURPOSE_START;

FOKL_HD bool emb_purpose_is_uniform(int purpose)
{
    return purpose == EMB_PURPOSE_ACCEPT || purpose == RES_PURPOSE_SIG_UNIFORM || purpose == RES_PURPOSE_TAU_UNIFORM ||
           purpose == RES_PURPOSE_START;
}

FOKL_HD void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t out[4])
{
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0, c1 = n1, c2 = n2, c3 = n3;
        k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
    }
    out[0] = c0, out[1] = c1, out[2] = c2, out[3] = c3;
}

FOKL_HD double emb_unit(uint32_t hi, uint32_t lo)
{
    return ((double)(hi >> 5) * 67108864.0 + (double)(lo >> 6)) * (1.0 / 9007199254740992.0);
}

FOKL_HD double emb_uniform(uint32_t seed, uint32_t chain, uint32_t draw, uint32_t purpose, uint32_t index)
{
    uint32_t w[4];
    philox4x32_10(draw, purpose, index, 0u, seed, chain, w);
    return emb_unit(w[0], w[1]);
}

// fokl_infer_device.inc / infer.py: the ensemble sampler over unknown inputs.  key = (seed, posterior draw), counter =
// (iteration, purpose, index, 1): the fourth word keeps these streams apart from every one above, which all use 0.
constexpr int INF_PURPOSE_PARTNER = 0;    // u1 of walker `index`: the partner (stretch), the first donor (jump)
constexpr int INF_PURPOSE_STRETCH = 1;    // u2: the stretch factor, the second donor
constexpr int INF_PURPOSE_ACCEPT = 2;     // u3: the accept uniform
constexpr int INF_PURPOSE_JITTER = 3;     // the jump move's normal of coordinate i of walker w, index 64 i + w
constexpr int INF_PURPOSE_LAST = INF_PURPOSE_JITTER;

FOKL_HD double inf_uniform(uint32_t seed, uint32_t draw_id, uint32_t iteration, uint32_t purpose, uint32_t index)
{
    uint32_t w[4];
    philox4x32_10(iteration, purpose, index, 1u, seed, draw_id, w);
    return emb_unit(w[0], w[1]);
}

FOKL_HD double inf_normal(uint32_t seed, uint32_t draw_id, uint32_t iteration, uint32_t purpose, uint32_t index)
{
    uint32_t w[4];
    philox4x32_10(iteration, purpose, index, 1u, seed, draw_id, w);
    return sqrt(-2.0 * log(1.0 - emb_unit(w[0], w[1]))) * cos(6.283185307179586476925 * emb_unit(w[2], w[3]));
}

// fokl_assimilate_device.inc / dynamics.assimilate: the bootstrap particle filter.  key = (seed, posterior draw), counter =
// (step, purpose, index, 2): the fourth word keeps these streams apart from every one above (0 and 1).  `step` is the point
// of the time axis the number is drawn for; purposes 0 .. 7 are the process noise of state j (index = particle).
constexpr int ASM_PURPOSE_INIT = 8;       // step 0: the normal that spreads particle i of state j at point 0, index 64 j + i
constexpr int ASM_PURPOSE_RESAMPLE = 9;   // the uniform of the systematic resampling at point `step` (index 0)
constexpr int ASM_PURPOSE_DRAW_INDEX = 10;   // draw id 0, step 0, index 0: the uniform behind the result's draw_index
constexpr int ASM_PURPOSE_LAST = ASM_PURPOSE_DRAW_INDEX;

FOKL_HD double asm_uniform(uint32_t seed, uint32_t draw_id, uint32_t step, uint32_t purpose, uint32_t index)
{
    uint32_t w[4];
    philox4x32_10(step, purpose, index, 2u, seed, draw_id, w);
    return emb_unit(w[0], w[1]);
}

FOKL_HD double asm_normal(uint32_t seed, uint32_t draw_id, uint32_t step, uint32_t purpose, uint32_t index)
{
    uint32_t w[4];
    philox4x32_10(step, purpose, index, 2u, seed, draw_id, w);
    return sqrt(-2.0 * log(1.0 - emb_unit(w[0], w[1]))) * cos(6.283185307179586476925 * emb_unit(w[2], w[3]));
}

// fokl_calibrate_device.inc / dynamics.calibrate: the ensemble sampler over the unknowns of a dynamic system, 128 walkers.
// key = (seed, posterior draw), counter = (iteration, purpose, index, 3): the fourth word keeps these streams apart from
// every one above (0, 1 and 2).  The purposes are the ensemble sampler's (INF_PURPOSE_*): u1, u2, u3 with index = walker
// 0 .. 127, and the jump move's normal of coordinate i of walker w with index 128 i + w.
FOKL_HD double cal_uniform(uint32_t seed, uint32_t draw_id, uint32_t iteration, uint32_t purpose, uint32_t index)
{
    uint32_t w[4];
    philox4x32_10(iteration, purpose, index, 3u, seed, draw_id, w);
    return emb_unit(w[0], w[1]);
}

FOKL_HD double cal_normal(uint32_t seed, uint32_t draw_id, uint32_t iteration, uint32_t purpose, uint32_t index)
{
    uint32_t w[4];
    philox4x32_10(iteration, purpose, index, 3u, seed, draw_id, w);
    return sqrt(-2.0 * log(1.0 - emb_unit(w[0], w[1]))) * cos(6.283185307179586476925 * emb_unit(w[2], w[3]));
}

// fokl_robust_device.inc / robust.py: Gibbs chains under Student-t noise.  key = (seed, chain), counter = (iteration,
// purpose + 16 attempt, index, 4): the fourth word keeps these streams apart from every one above (0 .. 3).
constexpr int ROB_PURPOSE_LAM_NORMAL = 0;    // the latent precision of row `index`: the normal of Marsaglia-Tsang attempt `attempt` ...
constexpr int ROB_PURPOSE_LAM_UNIFORM = 1;   // ... and its uniform
constexpr int ROB_PURPOSE_BETA = 2;          // the normal z of coordinate `index`
constexpr int ROB_PURPOSE_SIG_NORMAL = 3;    // sigma^2's gamma (index 0): the normal of attempt `attempt` ...
constexpr int ROB_PURPOSE_SIG_UNIFORM = 4;   // ... and its uniform
constexpr int ROB_PURPOSE_TAU_NORMAL = 5;    // tau^2's gamma: the same two
constexpr int ROB_PURPOSE_TAU_UNIFORM = 6;
constexpr int ROB_PURPOSE_LAST = ROB_PURPOSE_TAU_UNIFORM;
constexpr int ROB_ATTEMPT_STRIDE = 16;       // purpose word = purpose + 16 attempt

FOKL_HD bool rob_purpose_is_uniform(int purpose)
{
    return purpose == ROB_PURPOSE_LAM_UNIFORM || purpose == ROB_PURPOSE_SIG_UNIFORM || purpose == ROB_PURPOSE_TAU_UNIFORM;
}

FOKL_HD double rob_uniform(uint32_t seed, uint32_t chain, uint32_t iteration, uint32_t purpose_word, uint32_t index)
{
    uint32_t w[4];
    philox4x32_10(iteration, purpose_word, index, 4u, seed, chain, w);
    return emb_unit(w[0], w[1]);
}

FOKL_HD double rob_normal(uint32_t seed, uint32_t chain, uint32_t iteration, uint32_t purpose_word, uint32_t index)
{
    uint32_t w[4];
    philox4x32_10(iteration, purpose_word, index, 4u, seed, chain, w);
    return sqrt(-2.0 * log(1.0 - emb_unit(w[0], w[1]))) * cos(6.283185307179586476925 * emb_unit(w[2], w[3]));
}

FOKL_HD double emb_normal(uint32_t seed, uint32_t chain, uint32_t draw, uint32_t purpose, uint32_t index)
{
    uint32_t w[4];
    philox4x32_10(draw, purpose, index, 0u, seed, chain, w);
    return sqrt(-2.0 * log(1.0 - emb_unit(w[0], w[1]))) * cos(6.283185307179586476925 * emb_unit(w[2], w[3]));
}

}  // namespace fokl

#endif

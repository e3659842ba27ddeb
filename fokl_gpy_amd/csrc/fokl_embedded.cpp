// The host's view of the embedded-GP sampler's random numbers (fokl_philox.h): embedded.full_sample_host draws through
// this entry what hmc_chain_kernel draws on the device, so a transition can be compared value for value.
#include <cstdint>

#include "../../include/fokl_hip_internal.h"
#include "fokl_philox.h"

extern "C" int fokl_embedded_rng(uint32_t seed, uint32_t chain, uint32_t draw, int purpose, int count, double *out)
{
    if (count < 0 || (count > 0 && !out) || purpose < fokl::EMB_PURPOSE_MOMENTUM || purpose > fokl::EMB_PURPOSE_LAST)
        return FOKL_ERR_ARG;
    for (int j = 0; j < count; ++j)
        out[j] = fokl::emb_purpose_is_uniform(purpose) ? fokl::emb_uniform(seed, chain, draw, (uint32_t)purpose, (uint32_t)j)
                                                       : fokl::emb_normal(seed, chain, draw, (uint32_t)purpose, (uint32_t)j);
    return FOKL_OK;
}

// ... and of the ensemble sampler over unknown inputs (fokl_infer_device.inc; infer.sample_host draws through this entry)
extern "C" int fokl_infer_rng(uint32_t seed, uint32_t draw_id, uint32_t iteration, int purpose, int count, double *out)
{
    if (count < 0 || (count > 0 && !out) || purpose < fokl::INF_PURPOSE_PARTNER || purpose > fokl::INF_PURPOSE_LAST)
        return FOKL_ERR_ARG;
    for (int j = 0; j < count; ++j)
        out[j] = purpose == fokl::INF_PURPOSE_JITTER ? fokl::inf_normal(seed, draw_id, iteration, (uint32_t)purpose, (uint32_t)j)
                                                     : fokl::inf_uniform(seed, draw_id, iteration, (uint32_t)purpose, (uint32_t)j);
    return FOKL_OK;
}

// ... and of the particle filter over a fitted dynamic system (fokl_assimilate_device.inc; dynamics.assimilate_host draws
// through this entry): out [n_draws][count], one row per draw id
extern "C" int fokl_assimilate_rng(uint32_t seed, const uint32_t *draw_ids, int n_draws, uint32_t step, int purpose, int count,
                                   double *out)
{
    if (count < 0 || n_draws < 0 || (n_draws > 0 && !draw_ids) || (count > 0 && n_draws > 0 && !out) || purpose < 0 ||
        purpose > fokl::ASM_PURPOSE_LAST)
        return FOKL_ERR_ARG;
    const bool uniform = purpose == fokl::ASM_PURPOSE_RESAMPLE || purpose == fokl::ASM_PURPOSE_DRAW_INDEX;
    for (int e = 0; e < n_draws; ++e)
        for (int j = 0; j < count; ++j)
            out[(size_t)e * count + j] = uniform ? fokl::asm_uniform(seed, draw_ids[e], step, (uint32_t)purpose, (uint32_t)j)
                                                 : fokl::asm_normal(seed, draw_ids[e], step, (uint32_t)purpose, (uint32_t)j);
    return FOKL_OK;
}

// ... and of the calibration of such a system (fokl_calibrate_device.inc; dynamics.calibrate_host draws through this entry):
// out [n_draws][count], one row per draw id
extern "C" int fokl_calibrate_rng(uint32_t seed, const uint32_t *draw_ids, int n_draws, uint32_t iteration, int purpose, int count,
                                  double *out)
{
    if (count < 0 || n_draws < 0 || (n_draws > 0 && !draw_ids) || (count > 0 && n_draws > 0 && !out) ||
        purpose < fokl::INF_PURPOSE_PARTNER || purpose > fokl::INF_PURPOSE_LAST)
        return FOKL_ERR_ARG;
    for (int e = 0; e < n_draws; ++e)
        for (int j = 0; j < count; ++j)
            out[(size_t)e * count + j] = purpose == fokl::INF_PURPOSE_JITTER
                                             ? fokl::cal_normal(seed, draw_ids[e], iteration, (uint32_t)purpose, (uint32_t)j)
                                             : fokl::cal_uniform(seed, draw_ids[e], iteration, (uint32_t)purpose, (uint32_t)j);
    return FOKL_OK;
}

// ... and of the robust resampler (fokl_robust_device.inc; robust.pass_host / step_host draw through this entry): the numbers
// of indices first .. first + count - 1 at Marsaglia-Tsang attempt `attempt` (0 for the coordinates' normals)
extern "C" int fokl_robust_rng(uint32_t seed, uint32_t chain, uint32_t iteration, int purpose, int attempt, uint32_t first,
                               int64_t count, double *out)
{
    if (count < 0 || (count > 0 && !out) || purpose < fokl::ROB_PURPOSE_LAM_NORMAL || purpose > fokl::ROB_PURPOSE_LAST ||
        attempt < 0 || attempt > (1 << 20))
        return FOKL_ERR_ARG;
    const uint32_t word = (uint32_t)purpose + (uint32_t)fokl::ROB_ATTEMPT_STRIDE * (uint32_t)attempt;
    const bool uniform = fokl::rob_purpose_is_uniform(purpose);
    for (int64_t j = 0; j < count; ++j)
        out[j] = uniform ? fokl::rob_uniform(seed, chain, iteration, word, first + (uint32_t)j)
                         : fokl::rob_normal(seed, chain, iteration, word, first + (uint32_t)j);
    return FOKL_OK;
}

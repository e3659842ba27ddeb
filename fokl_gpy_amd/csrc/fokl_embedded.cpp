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

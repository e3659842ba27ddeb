// Host-only stand-ins for what the host translation units (sampler, thread pool, vector log, integrator) expect from
// fokl_hip.hip: the error plumbing and the version call.  Linked into the sanitizer builds of the host side
// (`make host-tsan host-asan`, tools/sanitize_host.sh) -- GPU sanitizers are not available on this pool, and the
// hand-rolled lock-free pipeline of fokl_hostpool.cpp is exactly the part that wants a race detector.  Device entry
// points are absent from those libraries: _capi.load() skips them when FOKL_HOST_ONLY_LIBRARY=1.
#include <cstdint>
#include <mutex>
#include <string>

#include "../../include/fokl_hip_internal.h"

static std::mutex g_err_mutex;
static std::string g_err;

void fokl_set_global_error(const std::string &msg)
{
    std::lock_guard<std::mutex> lock(g_err_mutex);
    g_err = msg;
}

extern "C" int fokl_version(void) { return 100; }

extern "C" __attribute__((visibility("hidden"))) int64_t fokl_dchain_dispatcher_cpu_ns() { return 0; }   // (no engine here)

extern "C" const char *fokl_last_error(const fokl_ctx *)
{
    std::lock_guard<std::mutex> lock(g_err_mutex);
    static thread_local std::string copy;
    copy = g_err;
    return copy.c_str();
}

extern "C" int fokl_device_count(int *count)
{
    if (count) *count = 0;
    return FOKL_ERR_HIP;
}

// GP_Integrate over an ensemble runs on the device only (fokl_integrate_device.inc); the single trajectory is host code.
extern "C" int fokl_gp_integrate_ensemble(fokl_ctx *, int, int, int, int64_t, const double *const *, const int32_t *,
                                          const int32_t *const *, const int32_t *, const int32_t *, const int32_t *const *,
                                          const int32_t *, const double *, const double *, const double *, int, int, double,
                                          const double *, int, int, double *, double *, double *)
{
    return FOKL_ERR_HIP;
}
extern "C" int fokl_gp_integrate_report(const fokl_ctx *, int64_t *) { return FOKL_ERR_HIP; }

// Neither does dynamics.simulate (fokl_simulate_device.inc); its statement is dynamics.simulate_host.
extern "C" int fokl_simulate_ensemble(fokl_ctx *, const fokl_system *, int, double *, double *, double *, int32_t *)
{
    return FOKL_ERR_HIP;
}
extern "C" int fokl_simulate_report(const fokl_ctx *, int64_t *) { return FOKL_ERR_HIP; }

// Nor its error-controlled sibling (fokl_simulate_adaptive_device.inc); its statement is dynamics.simulate_adaptive_host.
extern "C" int fokl_simulate_adaptive(fokl_ctx *, const fokl_system *, int, double, const double *, int, int, double *, double *, double *,
                                      int32_t *, int64_t *, int64_t *, int32_t *, double *, int32_t *, int8_t *)
{
    return FOKL_ERR_HIP;
}
extern "C" int fokl_simulate_adaptive_report(const fokl_ctx *, int64_t *) { return FOKL_ERR_HIP; }

// Nor the stiff sibling (fokl_simulate_stiff_device.inc); its statement is dynamics.simulate_stiff_host.
extern "C" int fokl_simulate_stiff(fokl_ctx *, const fokl_system *, int, double, const double *, int, int, double *, double *, double *,
                                   int32_t *, int64_t *, int64_t *, int64_t *, int32_t *, double *, int32_t *, int8_t *)
{
    return FOKL_ERR_HIP;
}
extern "C" int fokl_simulate_stiff_report(const fokl_ctx *, int64_t *) { return FOKL_ERR_HIP; }

// Nor the steady states of such a system (fokl_steady_device.inc); their statement is dynamics.steady_states_host.
extern "C" int fokl_steady_states(fokl_ctx *, const fokl_system *, const double *, int, int, double *, double *, int32_t *, int8_t *,
                                  int32_t *, uint8_t *, double *)
{
    return FOKL_ERR_HIP;
}
extern "C" int fokl_steady_report(const fokl_ctx *, int64_t *) { return FOKL_ERR_HIP; }

// Nor does the particle filter over such a system (fokl_assimilate_device.inc); its statement is dynamics.assimilate_host,
// and its random numbers (fokl_assimilate_rng) are host code and present here.
extern "C" int fokl_assimilate_ensemble(fokl_ctx *, const fokl_system *, const uint32_t *, int, const int32_t *, const double *, int,
                                        const int32_t *, const double *, const double *, const double *, const double *,
                                        double, uint32_t, double *, double *, double *, int32_t *, int32_t *)
{
    return FOKL_ERR_HIP;
}
extern "C" int fokl_assimilate_report(const fokl_ctx *, int64_t *) { return FOKL_ERR_HIP; }

// Nor does the calibration of such a system (fokl_calibrate_device.inc); its statement is dynamics.calibrate_host, and its
// random numbers (fokl_calibrate_rng) are host code and present here.
extern "C" int fokl_calibrate_ensemble(fokl_ctx *, const fokl_system *, const fokl_calibrate_problem *, double *, double *, int32_t *,
                                       double *, int32_t *, int64_t *, int32_t *, double *)
{
    return FOKL_ERR_HIP;
}
extern "C" int fokl_calibrate_report(const fokl_ctx *, int64_t *) { return FOKL_ERR_HIP; }

// Nor does the optimal control of such a system (fokl_control_device.inc); its statement is dynamics.control_host.
extern "C" int fokl_control_solve(fokl_ctx *, const fokl_system *, const fokl_control_problem *, double *, double *, double *,
                                  int32_t *, int32_t *, int32_t *, int32_t *, double *, int32_t *, double *, double *, double *)
{
    return FOKL_ERR_HIP;
}
extern "C" int fokl_control_report(const fokl_ctx *, int64_t *) { return FOKL_ERR_HIP; }

// Nor does the pooled solve over all draws (fokl_control_pooled_device.inc); its statement is dynamics.control_pooled_host.
extern "C" int fokl_control_pooled_solve(fokl_ctx *, const fokl_system *, const fokl_control_problem *, const double *, double *,
                                         double *, double *, int32_t *, int32_t *, int32_t *, int32_t *, double *, int32_t *,
                                         double *, double *, double *, const fokl_control_first_trial *)
{
    return FOKL_ERR_HIP;
}
extern "C" int fokl_control_pooled_report(const fokl_ctx *, int64_t *) { return FOKL_ERR_HIP; }

// Nor does the CVaR solve over all draws (fokl_control_cvar_device.inc); its statement is dynamics.control_cvar_host.
extern "C" int fokl_control_cvar_solve(fokl_ctx *, const fokl_system *, const fokl_control_problem *, const double *, double, double,
                                       double, double *, double *, double *, int32_t *, int32_t *, int32_t *, int32_t *, double *,
                                       int32_t *, double *, double *, double *, double *, double *, double *, double *,
                                       const fokl_control_first_trial *)
{
    return FOKL_ERR_HIP;
}
extern "C" int fokl_control_cvar_report(const fokl_ctx *, int64_t *) { return FOKL_ERR_HIP; }

// The multistart optimiser runs on the device only (fokl_optimize_device.inc on fokl_optimize_core.inc); its statement is
// optimize.solve_host.
extern "C" int fokl_model_optimize(fokl_ctx *, int, int, const int32_t *, int, const double *, const double *, int, int,
                                   const double *, const double *, int, const double *, double, int, double, double *,
                                   double *, int32_t *, int32_t *)
{
    return FOKL_ERR_HIP;
}

extern "C" int fokl_model_optimize_trace(fokl_ctx *, int, int, const int32_t *, int, const double *, const double *, int, int,
                                         const double *, const double *, int, const double *, double, int, double, double *,
                                         double *, int32_t *, int32_t *, int, double *)
{
    return FOKL_ERR_HIP;
}
extern "C" int fokl_optimize_report(const fokl_ctx *, int64_t *) { return FOKL_ERR_HIP; }

// Neither does the constrained optimiser over a system of models (fokl_optimize_system_device.inc;
// optimize.solve_system_host).
extern "C" int fokl_system_optimize(fokl_ctx *, int, int, const int32_t *, const int32_t *, const int32_t *, const int32_t *,
                                    const double *, const double *, int, const double *, const double *, int, int,
                                    const double *, const double *, int, const double *, int, int, double, double, double, int,
                                    const int32_t *, const int32_t *, const double *, int, double, double, double *, double *,
                                    double *, double *, double *, int32_t *, int32_t *)
{
    return FOKL_ERR_HIP;
}
extern "C" int fokl_system_optimize_trace(fokl_ctx *, int, int, const int32_t *, const int32_t *, const int32_t *,
                                          const int32_t *, const double *, const double *, int, const double *, const double *,
                                          int, int, const double *, const double *, int, const double *, int, int, double,
                                          double, double, int, const int32_t *, const int32_t *, const double *, int, double,
                                          double, double *, double *, double *, double *, double *, int32_t *, int32_t *, int,
                                          double *)
{
    return FOKL_ERR_HIP;
}
extern "C" int fokl_system_optimize_report(const fokl_ctx *, int64_t *) { return FOKL_ERR_HIP; }

// The embedded-GP sampler's chains run on the device only (fokl_embedded_device.inc); its statement is
// embedded.full_sample_host, and its random numbers (fokl_embedded_rng) are host code and present here.
extern "C" int fokl_embedded_hmc(fokl_ctx *, int, int, const int32_t *, int, const int32_t *, int, const int32_t *, int,
                                 const double *, int32_t, int, int, int, uint32_t, const double *, double, int, double *,
                                 double *, int32_t *, double *, double *, double *, int32_t *, double *, double *)
{
    return FOKL_ERR_HIP;
}
extern "C" int fokl_embedded_plan(int, int, int *, size_t *) { return FOKL_ERR_HIP; }

// A population through every posterior draw runs on the device only (fokl_population.inc); its statement is
// population.propagate_host.
extern "C" int fokl_population_stats(fokl_ctx *, const int32_t *, int, const double *, int, const double *, const double *,
                                     int, int, double *, int64_t *)
{
    return FOKL_ERR_HIP;
}
extern "C" int fokl_population_report(const fokl_ctx *, int64_t *) { return FOKL_ERR_HIP; }

// Neither do the resampler's chains (fokl_resample_device.inc); their statement is resample.resample_host.
extern "C" int fokl_resample_chains(fokl_ctx *, int, const double *, const double *, const double *, double, double, double,
                                    double, double, int, const double *, const double *, int, int, int, uint32_t, int, int,
                                    double *, double *, double *, int32_t *, double *, int64_t *)
{
    return FOKL_ERR_HIP;
}
extern "C" int fokl_resample_report(const fokl_ctx *, int64_t *) { return FOKL_ERR_HIP; }

// Nor do the robust chains (fokl_robust_device.inc); their statement is robust.robust_host, and their random numbers
// (fokl_robust_rng) are host code and present here.
extern "C" int fokl_robust_pass(fokl_ctx *, const int32_t *, int, const double *, int64_t, const double *, double, double, uint32_t,
                                uint32_t, uint32_t, int, double *, double *, int32_t *)
{
    return FOKL_ERR_HIP;
}
extern "C" int fokl_robust_step(fokl_ctx *, int, const double *, double, double, double, double, double, double, uint32_t, uint32_t,
                                uint32_t, int, double *, double *, int64_t *)
{
    return FOKL_ERR_HIP;
}
extern "C" int fokl_robust_chains(fokl_ctx *, const int32_t *, int, const double *, int64_t, double, double, double, double, double,
                                  const double *, int, const int32_t *, const double *, const double *, int, int, int, uint32_t,
                                  int, double *, double *, double *, int64_t *, double *, int64_t *, double *)
{
    return FOKL_ERR_HIP;
}
extern "C" int fokl_robust_report(const fokl_ctx *, int64_t *) { return FOKL_ERR_HIP; }

// Nor does the pointwise score (fokl_score_device.inc); its statement is score.score_rows_host.
extern "C" int fokl_score_rows(fokl_ctx *, const int32_t *, int, const double *, const double *, int, int, double *, double *)
{
    return FOKL_ERR_HIP;
}
extern "C" int fokl_score_rows_noise(fokl_ctx *, const int32_t *, int, const double *, const double *, int, int, double *, double *,
                                     double, const double *)
{
    return FOKL_ERR_HIP;
}
extern "C" int fokl_score_report(const fokl_ctx *, int64_t *) { return FOKL_ERR_HIP; }

// Nor does the predictive distribution per row (fokl_predictive_device.inc); its statement is predictive.predictive_rows_host.
extern "C" int fokl_predictive_rows(fokl_ctx *, const int32_t *, int, const double *, const double *, const double *, int, double,
                                    int, const double *, const double *, int, int, double, double, double *)
{
    return FOKL_ERR_HIP;
}
extern "C" int fokl_predictive_rows_noise(fokl_ctx *, const int32_t *, int, const double *, const double *, const double *, int,
                                          double, int, const double *, const double *, int, int, double, double, double *, double,
                                          const double *)
{
    return FOKL_ERR_HIP;
}
extern "C" int fokl_predictive_report(const fokl_ctx *, int64_t *) { return FOKL_ERR_HIP; }

// Nor does the greedy design over a pool (fokl_design_device.inc); its statement is design.select_host.
extern "C" int fokl_design_select(fokl_ctx *, const int32_t *, int, const double *, const double *, int, int, int, int, int64_t *,
                                  double *, double *, double *, double *, double *)
{
    return FOKL_ERR_HIP;
}
extern "C" int fokl_design_report(const fokl_ctx *, int64_t *) { return FOKL_ERR_HIP; }

// Nor does the batch acquisition over a pool (fokl_acquire_device.inc); its statement is acquire.select_host.
extern "C" int fokl_acquire_select(fokl_ctx *, const int32_t *, int, const double *, int, const double *, int, int, int, int, int,
                                   int64_t *, double *, double *, int64_t *, double *, unsigned char *)
{
    return FOKL_ERR_HIP;
}
extern "C" int fokl_acquire_report(const fokl_ctx *, int64_t *) { return FOKL_ERR_HIP; }

// ... nor under limits on other models' outputs (fokl_acquire_system_device.inc); acquire.select_system_host.
extern "C" int fokl_acquire_system_select(fokl_ctx *, const int32_t *, const int32_t *, int, const double *, int, const double *,
                                          const double *, const double *, int, int, int, int, int, int64_t *, double *, double *,
                                          int64_t *, int64_t *, double *, unsigned char *)
{
    return FOKL_ERR_HIP;
}
extern "C" int fokl_acquire_system_incumbent(fokl_ctx *, const int32_t *, const int32_t *, int, const double *, int, const double *,
                                             const double *, int, double *, int64_t *)
{
    return FOKL_ERR_HIP;
}
extern "C" int fokl_acquire_system_report(const fokl_ctx *, int64_t *) { return FOKL_ERR_HIP; }

// Nor do every draw's best rows of a pool (fokl_drawbest_device.inc); their statement is pooloptimum.ranks_host.
extern "C" int fokl_drawbest_rows(fokl_ctx *, const int32_t *, int, const double *, int, const unsigned char *, int, int, int64_t *,
                                  double *)
{
    return FOKL_ERR_HIP;
}
extern "C" int fokl_drawbest_report(const fokl_ctx *, int64_t *) { return FOKL_ERR_HIP; }

// Nor does the ensemble sampler over unknown inputs (fokl_infer_device.inc); its statement is infer.sample_host, and its
// random numbers (fokl_infer_rng) are host code and present here.
extern "C" int fokl_infer_inputs(fokl_ctx *, int, int, const int32_t *, int, const double *, const double *, const uint32_t *,
                                 const double *, int, int, const double *, const double *, const double *, const double *, int,
                                 const double *, const double *, const double *, int, int, int, int, uint32_t, int64_t,
                                 double *, double *, double *, int32_t *, int64_t *)
{
    return FOKL_ERR_HIP;
}
extern "C" int fokl_infer_report(const fokl_ctx *, int64_t *) { return FOKL_ERR_HIP; }

// The device chain engine and page-locked memory do not exist in these builds: the native search (fokl_search.cpp) is
// then created without an engine and falls back to ordinary memory for its tapes.
extern "C" int fokl_host_alloc(size_t, void **out)
{
    if (out) *out = nullptr;
    return FOKL_ERR_HIP;
}
extern "C" int fokl_host_free(void *) { return FOKL_ERR_HIP; }
extern "C" int fokl_dchain_submit(fokl_dchain *, int, int, const double *, const double *, double, double, double, double,
                                  double, const double *, const int32_t *, const double *, const double *, const int32_t *,
                                  const int32_t *, int, int, int, int64_t *, const double **)
{
    return FOKL_ERR_HIP;
}
extern "C" int fokl_dchain_submit_rows(fokl_dchain *, int, int, const double *, const double *, double, double, double, double,
                                       double, double, double, const fokl_tape_row *, const double *, const double *,
                                       const int32_t *, const uint64_t *, int, int64_t *, const double **)
{
    return FOKL_ERR_HIP;
}
extern "C" int fokl_dchain_wait(fokl_dchain *, int64_t, double *) { return FOKL_ERR_HIP; }
extern "C" int fokl_dchain_fetch_w(fokl_dchain *, int64_t, double *) { return FOKL_ERR_HIP; }
extern "C" int fokl_dchain_release(fokl_dchain *, int64_t) { return FOKL_ERR_HIP; }
extern "C" int fokl_dchain_try_release(fokl_dchain *, int64_t) { return 1; }
extern "C" int fokl_dchain_flush(fokl_dchain *) { return FOKL_ERR_HIP; }
// ... nor does the device's eigen-solver: a search in these builds is never bound to one.
extern "C" void fokl_device_dgemm(char *, char *, int *, int *, int *, double *, double *, int *, double *, int *, double *, double *,
                                  int *)
{
}
extern "C" int fokl_device_dgemm_configure(int, void *, int, void **) { return FOKL_ERR_HIP; }
extern "C" int fokl_device_dgemm_stats(int64_t *, int64_t *, int64_t *) { return FOKL_ERR_HIP; }
extern "C" int fokl_dspectral_max_columns(void) { return 0; }
extern "C" int fokl_dspectral_submit(fokl_dspectral *, const double *, int, const int32_t *, int, int, int, int64_t *, double **)
{
    return FOKL_ERR_HIP;
}
extern "C" int fokl_dspectral_flush(fokl_dspectral *) { return FOKL_ERR_HIP; }
extern "C" int fokl_dspectral_poll(fokl_dspectral *, int64_t) { return -FOKL_ERR_HIP; }
extern "C" int fokl_dspectral_wait(fokl_dspectral *, int64_t) { return FOKL_ERR_HIP; }
extern "C" int fokl_dspectral_release(fokl_dspectral *, int64_t) { return FOKL_ERR_HIP; }

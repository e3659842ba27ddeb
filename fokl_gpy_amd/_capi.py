"""
ctypes binding of libfokl_hip.so (C ABI: include/fokl_hip.h).

This is the only place the Python host code touches native code.  There is deliberately NO CPU fallback:
if the library is missing, or no gfx950 device is present when a device context is requested, the error
is raised to the caller.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('FOKL_HIP_LIBRARY', os.path.join(_HERE, 'libfokl_hip.so'))   # override: A/B builds

UNIQUE_ID_BYTES = 128
K_BASIS, K_GRAM, K_RESID, K_PREDICT, K_RESID_MF, K_GRAM_MFMA, K_GRAM_REDUCE = 0, 1, 2, 3, 4, 5, 6
K_INTEGRATE, K_BAND = 7, 8
K_OPTIMIZE = 9
K_OPTIMIZE_SYSTEM = 10
K_POPULATION = 11
K_RESAMPLE = 12
K_SCORE = 13
K_INFER = 14
K_DESIGN = 15
K_PREDICTIVE = 16
K_ROBUST = 17
K_ACQUIRE = 18
K_ACQUIRE_SYSTEM = 19
K_DRAWBEST = 20
INTEGRATE_MAX_STATES = 4
RESID_TERMS_MAX_FACTORS = 32
RESID_TERMS_MAX_ORDER = 8
RESID_TERMS_LAYOUTS = ((8, 1), (16, 1), (8, 2), (4, 4), (2, 8), (8, 4), (16, 2), (4, 8))    # inputs x orders per input (csrc/fokl_hip.hip)
SLOT_ONES, SLOT_Y, SLOT_FIRST_FREE = 0, 1, 2
PREDICT_NONE, PREDICT_VALU_LDS, PREDICT_VALU_GLOBAL, PREDICT_MFMA = 0, 1, 2, 3     # fokl_predict_report's kernel ids
POPULATION_COEFFICIENTS = ('none', 'registers', 'table')      # fokl_population_report: where the draw coefficients lived
POPULATION_MAX_CUTS = 32
SCORE_INSTANCES = ('none', 'waic', 'waic_loo')                # fokl_score_report: the instance of score_kernel that ran
SCORE_MAX_TAIL = 512                      # fokl_score_rows: entries (M + 1) of a row's list of largest log ratios in LDS
PREDICTIVE_INSTANCES = ('none', 'pit', 'quantiles', 'pit_quantiles')   # fokl_predictive_report: what the launch computed
PREDICTIVE_MAX_QUANTILES = 8              # fokl_predictive_rows: quantiles of one call (registers of a lane)
NOISES = ('gaussian', 'gaussian_weighted', 'student')        # fokl_score_report / fokl_predictive_report: the noise instance
PREDICTIVE_NU_MAX = 64                    # fokl_predictive_rows_noise: the largest finite nu (FOKL_PREDICTIVE_NU_MAX)
PREDICTIVE_STUDENT_ITERATIONS = 40        # ... and the fixed bound of the t CDF's continued fraction, host and device
RESAMPLE_MAX_COLUMNS = 768                # fokl_resample_chains: 12 eigen-coordinates per lane
RESAMPLE_ATTEMPT_CAP = 64                 # Marsaglia-Tsang attempts per gamma variate
RESAMPLE_SEGMENTS = 3                     # per-chain sums: first half, second half, the odd last iteration
# fokl_embedded_rng's purposes of the resampler (csrc/fokl_philox.h)
RES_BETA, RES_SIG_NORMAL, RES_SIG_UNIFORM, RES_TAU_NORMAL, RES_TAU_UNIFORM, RES_START = 3, 4, 5, 6, 7, 8
ROBUST_MAX_COLUMNS = 127                  # fokl_robust_*: P + 1; [1 | X | y] fills eight 16-column blocks
# fokl_robust_rng's purposes (csrc/fokl_philox.h): the lam variate's normal / uniform (index = row), z (index = coordinate),
# the normal / uniform of sigma^2's and tau^2's gamma variates (index 0); the attempt rides in the purpose word
ROB_LAM_NORMAL, ROB_LAM_UNIFORM, ROB_BETA, ROB_SIG_NORMAL, ROB_SIG_UNIFORM, ROB_TAU_NORMAL, ROB_TAU_UNIFORM = 0, 1, 2, 3, 4, 5, 6
DESIGN_INSTANCES = ('none', 'variance', 'ivr')                # fokl_design_report: the instance of the design kernels that ran
DESIGN_MAX_COLUMNS = 768                  # fokl_design_select: a 16-row tile of basis values in LDS is 96 KiB
ACQUIRE_INSTANCES = ('none', 'ei', 'pi')                      # fokl_acquire_report / fokl_acquire_select's criterion
ACQUIRE_MAX_COLUMNS = 1280                # fokl_acquire_select: a 16-row tile of basis values in LDS is 160 KiB
ACQUIRE_SYSTEM_INSTANCES = ('none', 'ei', 'pi', 'incumbent')  # fokl_acquire_system_report: what the last call ran
ACQUIRE_SYSTEM_MAX_MODELS = 8             # fokl_acquire_system_*: the objective and up to 7 constraint models
DRAWBEST_INSTANCES = ('none', 'ran')                          # fokl_drawbest_report: whether the last call ran
DRAWBEST_MAX_RANKS = 64                  # fokl_drawbest_rows: one pass over the pool per rank
DRAWBEST_MAX_COLUMNS = 1280               # ... and a 16-row tile of basis values in LDS is 160 KiB
OPTIMIZE_INSTANCES = ('none', 'uniform', 'per_lane')         # fokl_optimize_report / fokl_system_optimize_report
OPTIMIZE_TRIALS = 31                                          # trial points of one arc search (optimize.MAX_HALVINGS + 1)
INFER_MAPPINGS = ('none', 'walker_per_lane')                  # fokl_infer_report: the lane mapping that ran
INFER_WALKERS = 64                        # fokl_infer_inputs: one ensemble is one wavefront
INFER_TERM_CAP = 1 << 33                  # ... and the term evaluations by a wavefront asked of one launch
INFER_U1, INFER_U2, INFER_U3, INFER_JITTER = 0, 1, 2, 3      # fokl_infer_rng's purposes (csrc/fokl_philox.h)
ASSIMILATE_PARTICLES = 64                 # fokl_assimilate_ensemble: the particles of one draw are one wavefront
# fokl_assimilate_rng's purposes (csrc/fokl_philox.h); 0 .. 7 are the process-noise normals of state j
ASSIMILATE_INIT, ASSIMILATE_RESAMPLE, ASSIMILATE_DRAW_INDEX = 8, 9, 10
CALIBRATE_WALKERS = 128                   # fokl_calibrate_ensemble: an ensemble is two halves of one wavefront's 64 lanes
CALIBRATE_MAX_UNKNOWN = 16
# fokl_fit_report's kernel names, by id: Gram / residual / basis launch
GRAM_KERNELS = ('none', 'valu', 'tiles', 'dma', 'panel', 'tiles4')
RESID_KERNELS = ('none', 'columns', 'matrix_free')
BASIS_KERNELS = ('none', 'reg_table', 'lds_table')

c_int, c_i32, c_i64, c_dbl, c_vp = ctypes.c_int, ctypes.c_int32, ctypes.c_int64, ctypes.c_double, ctypes.c_void_p

# name -> (restype, argtypes); mirrors include/fokl_hip.h one to one (tests/test_capi_symbols.py checks it)
SIGNATURES = {
    'fokl_version': (c_int, []),
    'fokl_device_count': (c_int, [c_vp]),
    'fokl_ctx_create': (c_int, [c_int, c_vp]),
    'fokl_ctx_destroy': (None, [c_vp]),
    'fokl_last_error': (ctypes.c_char_p, [c_vp]),
    'fokl_sync': (c_int, [c_vp]),
    'fokl_upload': (c_int, [c_vp, c_vp, c_vp, c_i64, c_int, c_int, c_vp, c_int, c_int]),
    'fokl_stage_inputs': (c_int, [c_vp, c_vp, c_i64, c_int, c_vp, c_vp]),
    'fokl_upload_staged': (c_int, [c_vp, c_vp, c_i64, c_int, c_int, c_vp, c_int, c_int, c_vp, c_vp]),
    'fokl_download_inputs': (c_int, [c_vp, c_vp]),
    'fokl_column_min_max': (c_int, [c_vp, c_i64, c_int, c_vp, c_vp, c_int]),
    'fokl_normalize_columns': (c_int, [c_vp, c_i64, c_int, c_vp, c_vp, c_int]),
    'fokl_reserve_slots': (c_int, [c_vp, c_int]),
    'fokl_slot_capacity': (c_int, [c_vp]),
    'fokl_rows': (c_i64, [c_vp]),
    'fokl_build_terms': (c_int, [c_vp, c_vp, c_int, c_vp]),
    'fokl_build_terms_deriv': (c_int, [c_vp, c_vp, c_int, c_vp, c_int, c_int, c_dbl]),
    'fokl_gram': (c_int, [c_vp, c_vp, c_int, c_vp, c_int, c_vp, c_int, c_int]),
    'fokl_gram_launch': (c_int, [c_vp, c_vp, c_int, c_vp, c_int, c_int]),
    'fokl_gram_fetch': (c_int, [c_vp, c_vp, c_i64]),
    'fokl_gram_ready': (c_int, [c_vp]),
    'fokl_gram_plan': (c_int, [c_vp, c_int, c_vp, c_int, c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_int]),
    'fokl_bic_resid': (c_int, [c_vp, c_vp, c_int, c_vp, c_vp, c_int]),
    'fokl_bic_resid_launch': (c_int, [c_vp, c_vp, c_int, c_vp]),
    'fokl_bic_resid_fetch': (c_int, [c_vp, c_vp, c_int]),
    'fokl_bic_resid_terms_launch': (c_int, [c_vp, c_vp, c_int, c_vp]),
    'fokl_predict': (c_int, [c_vp, c_vp, c_int, c_vp, c_int, c_int, c_vp, c_vp]),
    'fokl_predict_report': (c_int, [c_vp, c_vp]),
    'fokl_fit_report': (c_int, [c_vp, c_int, c_vp, c_int]),
    'fokl_population_stats': (c_int, [c_vp, c_vp, c_int, c_vp, c_int, c_vp, c_vp, c_int, c_int, c_vp, c_vp]),
    'fokl_population_report': (c_int, [c_vp, c_vp]),
    'fokl_resample_chains': (c_int, [c_vp, c_int, c_vp, c_vp, c_vp, c_dbl, c_dbl, c_dbl, c_dbl, c_dbl, c_int, c_vp, c_vp, c_int,
                                     c_int, c_int, ctypes.c_uint32, c_int, c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    'fokl_resample_report': (c_int, [c_vp, c_vp]),
    'fokl_robust_pass': (c_int, [c_vp, c_vp, c_int, c_vp, c_i64, c_vp, c_dbl, c_dbl, ctypes.c_uint32, ctypes.c_uint32,
                                 ctypes.c_uint32, c_int, c_vp, c_vp, c_vp]),
    'fokl_robust_step': (c_int, [c_vp, c_int, c_vp, c_dbl, c_dbl, c_dbl, c_dbl, c_dbl, c_dbl, ctypes.c_uint32, ctypes.c_uint32,
                                 ctypes.c_uint32, c_int, c_vp, c_vp, c_vp]),
    'fokl_robust_chains': (c_int, [c_vp, c_vp, c_int, c_vp, c_i64, c_dbl, c_dbl, c_dbl, c_dbl, c_dbl, c_vp, c_int, c_vp, c_vp,
                                   c_vp, c_int, c_int, c_int, ctypes.c_uint32, c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    'fokl_robust_report': (c_int, [c_vp, c_vp]),
    'fokl_robust_rng': (c_int, [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, c_int, c_int, ctypes.c_uint32, c_i64, c_vp]),
    'fokl_score_rows': (c_int, [c_vp, c_vp, c_int, c_vp, c_vp, c_int, c_int, c_vp, c_vp]),
    'fokl_score_rows_noise': (c_int, [c_vp, c_vp, c_int, c_vp, c_vp, c_int, c_int, c_vp, c_vp, c_dbl, c_vp]),
    'fokl_score_report': (c_int, [c_vp, c_vp]),
    'fokl_predictive_rows': (c_int, [c_vp, c_vp, c_int, c_vp, c_vp, c_vp, c_int, c_dbl, c_int, c_vp, c_vp, c_int, c_int, c_dbl,
                                     c_dbl, c_vp]),
    'fokl_predictive_rows_noise': (c_int, [c_vp, c_vp, c_int, c_vp, c_vp, c_vp, c_int, c_dbl, c_int, c_vp, c_vp, c_int, c_int,
                                           c_dbl, c_dbl, c_vp, c_dbl, c_vp]),
    'fokl_predictive_report': (c_int, [c_vp, c_vp]),
    'fokl_design_select': (c_int, [c_vp, c_vp, c_int, c_vp, c_vp, c_int, c_int, c_int, c_int, c_vp, c_vp, c_vp, c_vp, c_vp,
                                   c_vp]),
    'fokl_design_report': (c_int, [c_vp, c_vp]),
    'fokl_acquire_select': (c_int, [c_vp, c_vp, c_int, c_vp, c_int, c_vp, c_int, c_int, c_int, c_int, c_int, c_vp, c_vp, c_vp,
                                    c_vp, c_vp, c_vp]),
    'fokl_acquire_report': (c_int, [c_vp, c_vp]),
    'fokl_acquire_system_select': (c_int, [c_vp, c_vp, c_vp, c_int, c_vp, c_int, c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int,
                                           c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    'fokl_acquire_system_incumbent': (c_int, [c_vp, c_vp, c_vp, c_int, c_vp, c_int, c_vp, c_vp, c_int, c_vp, c_vp]),
    'fokl_acquire_system_report': (c_int, [c_vp, c_vp]),
    'fokl_drawbest_rows': (c_int, [c_vp, c_vp, c_int, c_vp, c_int, c_vp, c_int, c_int, c_vp, c_vp]),
    'fokl_drawbest_report': (c_int, [c_vp, c_vp]),
    'fokl_read_slot': (c_int, [c_vp, c_int, c_i64, c_i64, c_vp]),
    'fokl_write_slot': (c_int, [c_vp, c_int, c_i64, c_i64, c_vp]),
    'fokl_timing_enable': (c_int, [c_vp, c_int]),
    'fokl_timing_reset': (c_int, [c_vp]),
    'fokl_timing_get': (c_int, [c_vp, c_int, c_vp, c_vp, c_vp, c_vp, c_vp]),
    'fokl_probe': (c_int, [c_vp, c_int, c_vp]),
    'fokl_gibbs_chain': (c_int, [c_vp, c_vp, c_int, c_dbl, c_dbl, c_dbl, c_dbl, c_dbl, c_dbl, c_dbl, c_int,
                                 c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    'fokl_noise_tape': (c_int, [c_int, c_int, c_dbl, c_dbl, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp,
                                c_vp]),
    'fokl_gibbs_chain_from_tape': (c_int, [c_vp, c_vp, c_int, c_dbl, c_dbl, c_dbl, c_dbl, c_dbl, c_int, c_vp, c_vp, c_vp,
                                           c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    'fokl_pool_create': (c_int, [c_int, c_int, c_int, c_int, c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_int, c_vp]),
    'fokl_pool_stream': (c_vp, [c_vp]),
    'fokl_pool_use_dsyevd': (c_int, [c_vp, c_vp, c_int]),
    'fokl_pool_use_dgemm': (c_int, [c_vp, c_vp]),
    'fokl_device_dgemm': (None, [c_vp] * 13),               # (called by the pool's threads through its address, not from here)
    'fokl_device_dgemm_configure': (c_int, [c_int, c_vp, c_int, c_vp]),
    'fokl_device_dgemm_stats': (c_int, [c_vp, c_vp, c_vp]),
    'fokl_pool_spectral_affinity': (c_int, [c_vp, c_vp, c_int]),
    'fokl_pool_release_hold': (c_int, [c_vp, ctypes.c_uint64]),
    'fokl_pool_destroy': (None, [c_vp]),
    'fokl_pool_submit_noise': (c_int, [c_vp, c_int, c_int, c_dbl, c_dbl, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_int,
                                       c_vp, c_int, c_int, c_vp, c_vp]),
    'fokl_tape_ready': (c_int, [c_vp, c_int, c_vp, c_int]),
    'fokl_pool_resolve': (c_int, [c_vp, c_int]),
    'fokl_pool_submit_chain': (c_int, [c_vp, c_vp, c_vp, c_int, c_dbl, c_dbl, c_dbl, c_dbl, c_dbl, c_int, c_vp, c_vp,
                                       c_vp, c_vp, c_vp, c_vp, c_vp, c_int, c_int, c_vp, c_vp, c_vp, c_vp, c_vp]),
    'fokl_pool_submit_spectral': (c_int, [c_vp, c_vp, c_int, c_vp, c_int, c_int, c_vp, c_vp, c_vp, c_vp, c_vp,
                                          c_vp]),
    'fokl_pool_submit_spectral_update': (c_int, [c_vp, c_vp, c_int, c_vp, c_int, c_int, c_vp, c_vp, c_int, c_vp, c_vp, c_vp,
                                                 c_vp, c_vp, c_vp, c_vp, c_vp]),
    'fokl_pool_poll': (c_int, [c_vp]),
    'fokl_pool_wait': (c_int, [c_vp]),
    'fokl_pool_busy_seconds': (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp]),
    'fokl_pool_noise_waits': (c_int, [c_vp, c_vp, c_vp]),
    'fokl_pool_chain_segments': (c_int, [c_vp, c_vp, c_vp]),
    'fokl_thread_cpu_seconds': (c_int, [c_vp, c_int]),
    'fokl_pool_stream_stats': (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    'fokl_stream_create': (c_int, [c_vp, c_i32, c_i32, c_dbl, c_int, c_vp, c_int, c_vp]),
    'fokl_stream_prestates_published': (c_i64, [c_vp]),
    'fokl_stream_given_gauss': (c_dbl, [c_vp]),
    'fokl_stream_destroy': (None, [c_vp]),
    'fokl_stream_walk': (c_int, [c_vp, c_int, c_int, c_dbl, c_dbl, c_vp, c_vp, c_vp, c_vp]),
    'fokl_stream_tell': (c_int, [c_vp, c_vp]),
    'fokl_stream_seek': (c_int, [c_vp, c_vp]),
    'fokl_stream_hold': (c_int, [c_vp, c_vp]),
    'fokl_stream_release': (c_int, [c_vp, ctypes.c_uint64]),
    'fokl_stream_advance_floor': (c_int, [c_vp]),
    'fokl_stream_state': (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp]),
    'fokl_stream_expand': (c_int, [c_vp, c_int, c_dbl, c_dbl, c_vp, c_int, c_int, c_vp, c_vp, c_vp, c_vp, c_vp]),
    'fokl_stream_stats': (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    'fokl_stream_set_helpers': (c_int, [c_vp, c_int, c_vp]),
    'fokl_stream_place_bulk': (c_int, [c_vp, c_vp, c_int]),
    'fokl_stream_fast_ln_error': (c_dbl, [c_i64]),
    'fokl_search_create': (c_int, [c_vp, c_vp, c_vp, c_vp]),
    'fokl_search_bind_spectral': (c_int, [c_vp, c_vp, c_int, c_dbl, c_int]),
    'fokl_search_hold_spectral': (c_int, [c_vp, c_int]),
    'fokl_search_set_update': (c_int, [c_vp, c_int, c_int, c_int]),
    'fokl_search_set_decide': (c_int, [c_vp, c_int, c_dbl]),
    'fokl_search_set_deterministic': (c_int, [c_vp, c_int]),
    'fokl_search_destroy': (None, [c_vp]),
    'fokl_search_error': (ctypes.c_char_p, [c_vp]),
    'fokl_search_mispredicted': (c_int, [c_vp]),
    'fokl_search_set_substage': (c_int, [c_vp, c_vp, c_int]),
    'fokl_search_speculate': (c_int, [c_vp, c_vp, c_vp, c_int]),
    'fokl_search_drop_speculation': (c_int, [c_vp]),
    'fokl_search_spectral': (c_int, [c_vp, c_vp, c_int, c_vp, c_int, c_vp]),
    'fokl_search_spectral_from': (c_int, [c_vp, c_vp, c_int, c_vp, c_int, c_vp, c_int, c_vp]),
    'fokl_spectrum_done': (c_int, [c_vp]),
    'fokl_spectrum_wait': (c_int, [c_vp, c_vp, c_vp, c_vp]),
    'fokl_spectrum_release': (None, [c_vp, c_vp]),
    'fokl_spectrum_retain': (c_int, [c_vp, c_vp]),
    'fokl_search_model_begin': (c_int, [c_vp, c_vp, c_int, c_vp, c_int, c_vp, c_vp, c_vp, c_int, c_vp, c_vp]),
    'fokl_search_model_request': (c_int, [c_vp, c_vp, c_int, c_vp, c_int, c_vp, c_vp, c_vp, c_int, c_vp, c_vp]),
    'fokl_search_model_abandon': (None, [c_vp, c_vp, c_vp]),
    'fokl_search_model_commit': (c_int, [c_vp, c_vp, c_vp, c_dbl, c_int, c_vp]),
    'fokl_run_create': (c_int, [c_vp, c_vp, c_vp]),
    'fokl_run_set_update': (c_int, [c_vp, c_int, c_int, c_int]),
    'fokl_run_search': (c_int, [c_vp, c_vp]),
    'fokl_run_result': (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    'fokl_run_arrays': (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    'fokl_run_order': (c_int, [c_vp, c_vp, c_int]),
    'fokl_run_error': (ctypes.c_char_p, [c_vp]),
    'fokl_run_destroy': (None, [c_vp]),
    'fokl_search_score': (c_int, [c_vp, c_vp, c_dbl, c_dbl, c_int, c_int, c_vp]),
    'fokl_outcome_info': (c_int, [c_vp, c_vp, c_vp]),
    'fokl_outcome_spectrum': (c_int, [c_vp, c_vp, c_vp]),
    'fokl_outcome_chain_ready': (c_int, [c_vp]),
    'fokl_outcome_draws': (c_int, [c_vp, c_vp, c_vp]),
    'fokl_outcome_intercept_scale': (c_int, [c_vp, c_vp, c_vp]),
    'fokl_outcome_new_term_stats': (c_int, [c_vp, c_vp, c_vp, c_int, c_int, c_int, c_vp, c_vp]),
    'fokl_outcome_release': (None, [c_vp, c_vp]),
    'fokl_outcome_drop': (None, [c_vp, c_vp]),
    'fokl_search_verify': (c_int, [c_vp, c_int]),
    'fokl_search_register_forecast': (c_int, [c_vp, c_vp, c_int, c_vp, c_dbl]),
    'fokl_search_clear_forecasts': (None, [c_vp]),
    'fokl_search_likely_first_tests': (c_int, [c_vp, c_vp, c_int, c_dbl, c_vp, c_vp, c_vp]),
    'fokl_search_stats': (c_int, [c_vp, c_vp, c_int]),
    'fokl_search_trace': (c_i64, [c_vp, c_vp, c_i64]),
    'fokl_search_kill_tests': (c_int, [c_vp, c_vp, c_vp]),
    'fokl_finish_tape_blocks': (c_int, [c_int, c_int, c_vp, c_vp, c_vp, c_vp, c_int, c_int, c_int, c_vp]),
    'fokl_gibbs_chain_from_finished_tape': (c_int, [c_vp, c_vp, c_int, c_dbl, c_dbl, c_dbl, c_dbl, c_dbl, c_int, c_vp,
                                                    c_vp, c_vp, c_vp, c_int, c_vp, c_vp, c_vp, c_vp]),
    'fokl_gibbs_chain_segments_host': (c_int, [c_vp, c_vp, c_int, c_dbl, c_dbl, c_dbl, c_dbl, c_dbl, c_int, c_vp, c_vp,
                                               c_vp, c_vp, c_int, c_vp, c_vp, c_vp, c_vp, c_int, c_int, c_vp]),
    'fokl_rng_normals': (c_int, [c_vp, c_vp, c_vp, c_vp, c_i64, c_vp]),
    'fokl_rng_gammas': (c_int, [c_vp, c_vp, c_vp, c_vp, c_dbl, c_dbl, c_i64, c_vp]),
    'fokl_gp_integrate': (c_int, [c_int, c_int, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_int, c_int,
                                  c_dbl, c_vp, c_vp]),
    'fokl_gp_integrate_ensemble': (c_int, [c_vp, c_int, c_int, c_int, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp,
                                           c_vp, c_vp, c_int, c_int, c_dbl, c_vp, c_int, c_int, c_vp, c_vp, c_vp]),
    'fokl_gp_integrate_report': (c_int, [c_vp, c_vp]),
    'fokl_simulate_ensemble': (c_int, [c_vp, c_vp, c_int, c_vp, c_vp, c_vp, c_vp]),
    'fokl_simulate_report': (c_int, [c_vp, c_vp]),
    'fokl_simulate_adaptive': (c_int, [c_vp, c_vp, c_int, c_dbl, c_vp, c_int, c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp,
                                       c_vp]),
    'fokl_simulate_adaptive_report': (c_int, [c_vp, c_vp]),
    'fokl_simulate_stiff': (c_int, [c_vp, c_vp, c_int, c_dbl, c_vp, c_int, c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp,
                                    c_vp]),
    'fokl_simulate_stiff_report': (c_int, [c_vp, c_vp]),
    'fokl_steady_states': (c_int, [c_vp, c_vp, c_vp, c_int, c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    'fokl_steady_report': (c_int, [c_vp, c_vp]),
    'fokl_assimilate_ensemble': (c_int, [c_vp, c_vp, c_vp, c_int, c_vp, c_vp, c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_dbl, ctypes.c_uint32,
                                         c_vp, c_vp, c_vp, c_vp, c_vp]),
    'fokl_assimilate_report': (c_int, [c_vp, c_vp]),
    'fokl_calibrate_ensemble': (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    'fokl_calibrate_report': (c_int, [c_vp, c_vp]),
    'fokl_calibrate_rng': (c_int, [ctypes.c_uint32, c_vp, c_int, ctypes.c_uint32, c_int, c_int, c_vp]),
    'fokl_control_solve': (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    'fokl_control_report': (c_int, [c_vp, c_vp]),
    'fokl_control_pooled_solve': (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp,
                                          c_vp]),
    'fokl_control_pooled_report': (c_int, [c_vp, c_vp]),
    'fokl_control_cvar_solve': (c_int, [c_vp, c_vp, c_vp, c_vp, c_dbl, c_dbl, c_dbl, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp,
                                        c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    'fokl_control_cvar_report': (c_int, [c_vp, c_vp]),
    'fokl_assimilate_rng': (c_int, [ctypes.c_uint32, c_vp, c_int, ctypes.c_uint32, c_int, c_int, c_vp]),
    'fokl_model_optimize': (c_int, [c_vp, c_int, c_int, c_vp, c_int, c_vp, c_vp, c_int, c_int, c_vp, c_vp, c_int, c_vp, c_dbl,
                                    c_int, c_dbl, c_vp, c_vp, c_vp, c_vp]),
    'fokl_system_optimize': (c_int, [c_vp, c_int, c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_int, c_vp, c_vp, c_int, c_int,
                                     c_vp, c_vp, c_int, c_vp, c_int, c_int, c_dbl, c_dbl, c_dbl, c_int, c_vp, c_vp, c_vp,
                                     c_int, c_dbl, c_dbl, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    'fokl_model_optimize_trace': (c_int, [c_vp, c_int, c_int, c_vp, c_int, c_vp, c_vp, c_int, c_int, c_vp, c_vp, c_int, c_vp,
                                          c_dbl, c_int, c_dbl, c_vp, c_vp, c_vp, c_vp, c_int, c_vp]),
    'fokl_system_optimize_trace': (c_int, [c_vp, c_int, c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_int, c_vp, c_vp, c_int,
                                           c_int, c_vp, c_vp, c_int, c_vp, c_int, c_int, c_dbl, c_dbl, c_dbl, c_int, c_vp, c_vp,
                                           c_vp, c_int, c_dbl, c_dbl, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_int, c_vp]),
    'fokl_optimize_report': (c_int, [c_vp, c_vp]),
    'fokl_system_optimize_report': (c_int, [c_vp, c_vp]),
    'fokl_embedded_hmc': (c_int, [c_vp, c_int, c_int, c_vp, c_int, c_vp, c_int, c_vp, c_int, c_vp, c_int, c_int, c_int, c_int,
                                  ctypes.c_uint32, c_vp, c_dbl, c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    'fokl_embedded_plan': (c_int, [c_int, c_int, c_vp, c_vp]),
    'fokl_embedded_rng': (c_int, [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, c_int, c_int, c_vp]),
    'fokl_infer_inputs': (c_int, [c_vp, c_int, c_int, c_vp, c_int, c_vp, c_vp, c_vp, c_vp, c_int, c_int, c_vp, c_vp, c_vp, c_vp,
                                  c_int, c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, ctypes.c_uint32, c_i64, c_vp, c_vp, c_vp,
                                  c_vp, c_vp]),
    'fokl_infer_report': (c_int, [c_vp, c_vp]),
    'fokl_infer_rng': (c_int, [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, c_int, c_int, c_vp]),
    'fokl_dchain_create': (c_int, [c_int, c_int, c_vp]),
    'fokl_dchain_destroy': (None, [c_vp]),
    'fokl_dchain_submit': (c_int, [c_vp, c_int, c_int, c_vp, c_vp, c_dbl, c_dbl, c_dbl, c_dbl, c_dbl, c_vp, c_vp, c_vp,
                                   c_vp, c_vp, c_vp, c_int, c_int, c_int, c_vp, c_vp]),
    'fokl_dchain_prestate_ring': (c_int, [c_vp, c_vp, c_vp]),
    'fokl_dchain_bind_stream': (c_int, [c_vp, c_vp]),
    'fokl_dchain_submit_rows': (c_int, [c_vp, c_int, c_int, c_vp, c_vp, c_dbl, c_dbl, c_dbl, c_dbl, c_dbl, c_dbl, c_dbl, c_vp,
                                        c_vp, c_vp, c_vp, c_vp, c_int, c_vp, c_vp]),
    'fokl_dchain_stream_stats': (c_int, [c_vp, c_vp, c_vp]),
    'fokl_dchain_try_release': (c_int, [c_vp, c_i64]),
    'fokl_dchain_poll': (c_int, [c_vp, c_i64]),
    'fokl_dchain_flush': (c_int, [c_vp]),
    'fokl_dchain_wait': (c_int, [c_vp, c_i64, c_vp]),
    'fokl_dchain_fetch_w': (c_int, [c_vp, c_i64, c_vp]),
    'fokl_dchain_release': (c_int, [c_vp, c_i64]),
    'fokl_dchain_stats': (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp]),
    'fokl_dchain_recuts': (c_int, [c_vp, c_vp]),
    'fokl_dspectral_create': (c_int, [c_int, c_vp]),
    'fokl_dspectral_destroy': (None, [c_vp]),
    'fokl_dspectral_max_columns': (c_int, []),
    'fokl_dspectral_set_signs': (c_int, [c_vp, c_int]),
    'fokl_dspectral_submit': (c_int, [c_vp, c_vp, c_int, c_vp, c_int, c_int, c_int, c_vp, c_vp]),
    'fokl_dspectral_flush': (c_int, [c_vp]),
    'fokl_dspectral_poll': (c_int, [c_vp, c_i64]),
    'fokl_dspectral_wait': (c_int, [c_vp, c_i64]),
    'fokl_dspectral_release': (c_int, [c_vp, c_i64]),
    'fokl_dspectral_stats': (c_int, [c_vp, c_vp, c_vp]),
    'fokl_host_alloc': (c_int, [ctypes.c_size_t, c_vp]),
    'fokl_host_free': (c_int, [c_vp]),
    'fokl_comm_unique_id': (c_int, [c_vp]),
    'fokl_comm_init': (c_int, [c_vp, c_vp, c_int, c_int]),
    'fokl_comm_destroy': (c_int, [c_vp]),
    'fokl_comm_init_detached': (c_int, [c_int, c_vp, c_int, c_int, ctypes.POINTER(c_vp)]),
    'fokl_comm_adopt': (c_int, [c_vp, c_vp, c_int, c_int]),
    'fokl_comm_release_detached': (c_int, [c_vp]),
    'fokl_comm_allgather_f64': (c_int, [c_vp, c_vp, c_int, c_vp]),
    'fokl_comm_allreduce_sum_f64': (c_int, [c_vp, c_vp, c_int]),
}


class FoklNativeError(RuntimeError):
    """A libfokl_hip call returned a non-zero status."""

    def __init__(self, code, message):
        super().__init__(f"libfokl_hip error {code}: {message}")
        self.code = code


_lib = None


def load():
    """Load libfokl_hip.so (built in-tree by ``__graft_entry__.build()`` / ``make -C fokl_gpy_amd/csrc``)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FoklNativeError(-1, f"{LIB_PATH} not found -- build it with `python -c 'import __graft_entry__ as g; "
                                  f"g.build()'` or `make -C fokl_gpy_amd/csrc` (there is no CPU fallback)")
    lib = ctypes.CDLL(LIB_PATH)
    host_only = os.environ.get('FOKL_HOST_ONLY_LIBRARY', '0') == '1'      # sanitizer builds of the host side (csrc/Makefile)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name, None) if host_only else getattr(lib, name)
        if fn is None:
            continue
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def _ptr(arr):
    """Address of a numpy buffer as a plain integer (accepted by every c_void_p parameter; far cheaper than
    ``arr.ctypes.data_as``, which showed up at 3 us a call on the search's critical thread)."""
    return arr.__array_interface__['data'][0] if arr is not None else None


def _check(rc, ctx=None):
    if rc != 0:
        msg = load().fokl_last_error(ctx)
        raise FoklNativeError(rc, msg.decode() if msg else "unknown error")


def embedded_rng(seed, chain, draw, purpose, count):
    """The numbers the embedded-GP sampler and the resampler draw (fokl_embedded_rng: Philox 4x32-10 keyed by (seed, chain),
    counter (draw, purpose, index); purposes 0 .. 2 the embedded sampler's, RES_* the resampler's); host code, no device."""
    out = np.empty(int(count), dtype=np.float64)
    _check(load().fokl_embedded_rng(int(seed) & 0xFFFFFFFF, int(chain), int(draw), int(purpose), int(count), _ptr(out)))
    return out


def robust_rng(seed, chain, iteration, purpose, count, attempt=0, first=0):
    """The numbers the robust resampler draws (fokl_robust_rng: Philox 4x32-10 keyed by (seed, chain), counter (iteration,
    purpose + 16 attempt, index, 4)) for the indices first .. first + count - 1; purposes ROB_*: uniforms for the *_UNIFORM
    ones, normals otherwise; host code, no device."""
    out = np.empty(int(count), dtype=np.float64)
    _check(load().fokl_robust_rng(int(seed) & 0xFFFFFFFF, int(chain), int(iteration), int(purpose), int(attempt), int(first),
                                  int(count), _ptr(out)))
    return out


def assimilate_rng(seed, draw_ids, step, purpose, count):
    """The numbers the particle filter draws (fokl_assimilate_rng: Philox 4x32-10 keyed by (seed, draw id), counter (step,
    purpose, index, 2)) -> [len(draw_ids), count]; purposes 0 .. 7 the process-noise normal of that state (index = particle),
    ASSIMILATE_INIT the start's normal (index 64 j + particle), ASSIMILATE_RESAMPLE and ASSIMILATE_DRAW_INDEX uniforms;
    host code, no device."""
    ids = np.ascontiguousarray(draw_ids, dtype=np.uint32)
    out = np.empty((ids.shape[0], int(count)), dtype=np.float64)
    _check(load().fokl_assimilate_rng(int(seed) & 0xFFFFFFFF, _ptr(ids), int(ids.shape[0]), int(step), int(purpose), int(count),
                                      _ptr(out)))
    return out


def calibrate_rng(seed, draw_ids, iteration, purpose, count):
    """The numbers ``dynamics.calibrate``'s sampler draws (fokl_calibrate_rng: Philox 4x32-10 keyed by (seed, draw id), counter
    (iteration, purpose, index, 3)) -> [len(draw_ids), count]; purposes INFER_U1 .. INFER_U3 uniforms of walker ``index``
    (0 .. 127), INFER_JITTER the normal of index 128 i + w; host code, no device."""
    ids = np.ascontiguousarray(draw_ids, dtype=np.uint32)
    out = np.empty((ids.shape[0], int(count)), dtype=np.float64)
    _check(load().fokl_calibrate_rng(int(seed) & 0xFFFFFFFF, _ptr(ids), int(ids.shape[0]), int(iteration), int(purpose),
                                     int(count), _ptr(out)))
    return out


def infer_rng(seed, draw_id, iteration, purpose, count):
    """The numbers the ensemble sampler over unknown inputs draws (fokl_infer_rng: Philox 4x32-10 keyed by (seed, draw_id),
    counter (iteration, purpose, index, 1); purposes INFER_U1 .. INFER_U3 uniforms of walker ``index``, INFER_JITTER the
    normal of index 64 i + w); host code, no device."""
    out = np.empty(int(count), dtype=np.float64)
    _check(load().fokl_infer_rng(int(seed) & 0xFFFFFFFF, int(draw_id), int(iteration), int(purpose), int(count), _ptr(out)))
    return out


def device_count():
    n = c_int(0)
    rc = load().fokl_device_count(ctypes.byref(n))
    return n.value if rc == 0 else 0


# ---------------------------------------------------------------------------------------------------------
# numpy legacy RNG state <-> the C sampler
# ---------------------------------------------------------------------------------------------------------

def gram_plan(row_slots, col_slots, kind=0):
    """fokl_gram_plan: the tile lists fokl_gram's MFMA path would use for this block (host arithmetic, no device);
    kind 0 = gram_tiles_kernel (16x16x4 MFMA; the default), kind 1 = gram_tiles4s_kernel (4x4x4 MFMA; FOKL_GRAM_MFMA4=2).
    -> dict(nci, i_tiles, j_tiles, nt, ct, rows_per_chunk, ks, depth, waves, icols, perm, staged [G, 16],
            tiles [G, 4, 10, 4] = (local row-side tile, local column-side tile, out i-tile, out j-tile; -1: padding),
            half [G, 4, 10] = entries of a ragged last row tile that gram_tiles_dma_kernel forms with 4x4x4 MFMAs)"""
    rs = np.ascontiguousarray(row_slots, dtype=np.int32)
    cs = np.ascontiguousarray(col_slots, dtype=np.int32)
    info = np.zeros(10, dtype=np.int32)
    lib = load()
    _check(lib.fokl_gram_plan(_ptr(rs), rs.shape[0], _ptr(cs), cs.shape[0], int(kind), _ptr(info), None, None, None,
                              None, 0))
    groups = int(info[3])
    icols = np.empty(int(info[0]), dtype=np.int32)
    perm = np.empty(cs.shape[0], dtype=np.int32)
    staged = np.empty((groups, 16), dtype=np.int32)
    tiles = np.empty((groups, 4, 10, 4), dtype=np.int32)
    _check(lib.fokl_gram_plan(_ptr(rs), rs.shape[0], _ptr(cs), cs.shape[0], int(kind), _ptr(info), _ptr(icols),
                              _ptr(perm), _ptr(staged), _ptr(tiles), groups))
    half = (tiles[..., 0] >= 256) & (tiles[..., 2] >= 0)       # entries the LDS-DMA kernel computes as half tiles
    tiles[..., 0] &= 255
    return dict(nci=int(info[0]), i_tiles=int(info[1]), j_tiles=int(info[2]), nt=int(info[4]), ct=int(info[5]),
                rows_per_chunk=32 << int(info[6]), ks=int(info[7]), depth=int(info[8]), waves=int(info[9]), icols=icols,
                perm=perm, staged=staged, tiles=tiles, half=half)


def device_dgemm_stats():
    """(calls of fokl_device_dgemm so far in this process, of which ran on the device, device attempts that fell back)"""
    v = [ctypes.c_int64(0) for _ in range(3)]
    if load().fokl_device_dgemm_stats(*[ctypes.byref(x) for x in v]) != 0:
        return 0, 0, 0
    return tuple(x.value for x in v)


class TraceRecords:
    """The evaluations of a search in order, one dict(cols, built, ev, kill, b0) each -- formed when somebody looks (a fit has
    hundreds of them and the search's last half millisecond is no place to build them)."""

    def __init__(self, rec):
        self._rec = rec

    def __len__(self):
        return self._rec.shape[0]

    @staticmethod
    def _record(r):
        return dict(cols=int(r[0]), built=int(r[1]), ev=float(r[2]), kill=bool(r[3]), b0=float(r[4]))

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self._record(r) for r in self._rec[i]]
        return self._record(self._rec[i])

    def __iter__(self):
        return (self._record(r) for r in self._rec)

    def __eq__(self, other):
        return list(self) == list(other)

    def __repr__(self):
        return repr(list(self))


class LegacyStream:
    """Mutable copy of numpy's global legacy RNG state in the layout the C sampler updates in place."""

    def __init__(self, state=None):
        st = np.random.get_state() if state is None else state
        if st[0] != 'MT19937':
            raise ValueError("numpy's global RNG is not MT19937")
        self.key = np.array(st[1], dtype=np.uint32, copy=True)
        self.pos = ctypes.c_int32(int(st[2]))
        self.has_gauss = ctypes.c_int32(int(st[3]))
        self.cache = ctypes.c_double(float(st[4]))

    def as_numpy_state(self):
        return ('MT19937', self.key.copy(), int(self.pos.value), int(self.has_gauss.value), float(self.cache.value))

    def publish(self):
        """Write the advanced state back to numpy's global generator."""
        np.random.set_state(self.as_numpy_state())

    def args(self):
        return (_ptr(self.key), ctypes.byref(self.pos), ctypes.byref(self.has_gauss), ctypes.byref(self.cache))

    def normals(self, n):
        out = np.empty(int(n), dtype=np.float64)
        _check(load().fokl_rng_normals(*self.args(), c_i64(int(n)), _ptr(out)))
        return out

    def gammas(self, shape, scale, n):
        out = np.empty(int(n), dtype=np.float64)
        _check(load().fokl_rng_gammas(*self.args(), c_dbl(shape), c_dbl(scale), c_i64(int(n)), _ptr(out)))
        return out


THREAD_KINDS = ('walker', 'chain', 'finish', 'spectral', 'bulk', 'device_chain_dispatcher')


def thread_cpu_seconds():
    """CPU-seconds used so far by the library's own threads, by kind (fokl_thread_cpu_seconds)."""
    v = np.zeros(8)
    n = load().fokl_thread_cpu_seconds(_ptr(v), v.shape[0])
    if n < 0:
        _check(n)
    return dict(zip(THREAD_KINDS, v[:n].tolist()))


def _host_threads():
    try:
        return max(1, min(8, len(os.sched_getaffinity(0))))
    except (AttributeError, OSError):
        return 1


def column_min_max(x):
    """(minima, maxima) of the columns of a C-contiguous float64 [n, m] array on several host threads (fokl_column_min_max:
    np.min / np.max per column, exact)."""
    n, m = x.shape
    lows, highs = np.empty(m), np.empty(m)
    _check(load().fokl_column_min_max(_ptr(x), n, m, _ptr(lows), _ptr(highs), _host_threads()))
    return lows, highs


def normalize_columns(x, lows, spans):
    """x <- (x - lows) / spans in place, element by element as numpy does it (fokl_normalize_columns)."""
    lows = np.ascontiguousarray(lows, dtype=np.float64)
    spans = np.ascontiguousarray(spans, dtype=np.float64)
    _check(load().fokl_normalize_columns(_ptr(x), x.shape[0], x.shape[1], _ptr(lows), _ptr(spans), _host_threads()))
    return x


def gibbs_chain(lamb, qty, astar, atau_star, b, btau, dtd, sigsqd0, tausqd0, draws, stream, want_sig_tau=False):
    """G3 in the eigenbasis (include/fokl_hip.h: fokl_gibbs_chain).  Returns w [draws, p1] (betas = w @ Q.T)."""
    lamb = np.ascontiguousarray(lamb, dtype=np.float64)
    qty = np.ascontiguousarray(qty, dtype=np.float64)
    p1 = lamb.shape[0]
    w = np.empty((int(draws), p1), dtype=np.float64)
    sigs = np.empty(int(draws)) if want_sig_tau else None
    taus = np.empty(int(draws)) if want_sig_tau else None
    _check(load().fokl_gibbs_chain(_ptr(lamb), _ptr(qty), p1, float(astar), float(atau_star), float(b), float(btau),
                                   float(dtd), float(sigsqd0), float(tausqd0), int(draws), *stream.args(),
                                   _ptr(w), _ptr(sigs), _ptr(taus)))
    if want_sig_tau:
        return w, sigs, taus
    return w


class NoiseTape:
    """The data-independent random numbers of one candidate's chain (include/fokl_hip.h: fokl_noise_tape): per
    iteration p1 normals -- accepted polar pairs left unfinished, see the header -- and two standard gammas.
    ``progress[0]`` counts the iterations recorded so far (-1 = the producer failed); ``block_done`` are the flags of
    fokl_finish_tape_blocks (blocks of BLOCK iterations).
    One allocation, carved up by address: a tape is made for every model evaluation on the search's critical thread."""
    __slots__ = ('p1', 'draws', 'finishing_requested', 'materialised_by_pool', '_buf', '_addr', '_off', '_ints')
    BLOCK = 16                                                # = FOKL_TAPE_BLOCK

    @classmethod
    def _layout(cls, p1, d):
        half = p1 // 2 + 1
        nblocks = -(-d // cls.BLOCK)
        pad = lambda count: -(-count // 8) * 8                # regions start on 64-byte lines (in doubles)
        # int32 area: progress (a line of its own: polled by other threads) | block_done [nblocks] | lead [d]
        ints = (16, 16 + -(-nblocks // 16) * 16)
        off = [0]
        for count in (d * p1 + 16, d * half + 8, d, d):     # slack: the recorder stores whole vectors (see the header)
            off.append(off[-1] + pad(count))
        # behind the int32 area: the tape as the pool's walker leaves it (fokl_tape_row [d]: 4 x uint64 each)
        rows = off[4] + pad((ints[1] + d + 1) // 2) + 8
        off.append(rows)
        return tuple(off), ints, rows + 4 * d + 8

    @classmethod
    def doubles_needed(cls, p1, draws):
        return cls._layout(int(p1), int(draws))[2]

    def __init__(self, p1, draws, raw=None):
        """raw: a float64 buffer of at least doubles_needed(p1, draws) elements to build the tape in (recycled memory
        is already mapped and probably cached), else a fresh allocation."""
        self.p1, self.draws = p1, d = int(p1), int(draws)
        off, ints, total = self._layout(p1, d)
        self._off, self._ints = off, ints
        if raw is None:
            raw = np.empty(total, dtype=np.float64)
        elif raw.shape[0] < total:
            raise ValueError("buffer too small for this tape")
        shift = ((-raw.__array_interface__['data'][0]) % 64) // 8
        self._buf = raw[shift:]
        self._addr = self._buf.__array_interface__['data'][0]
        self._buf[off[4]:off[4] + ints[1] // 2] = 0.0         # progress and block flags start at zero
        self.finishing_requested = False                      # HostPool.submit_noise(..., finish=True) was given this tape
        self.materialised_by_pool = False                     # block_done flags: set by the pool's finish threads

    def _int_area(self):
        return self._buf[self._off[4]:].view(np.int32)

    normals = property(lambda self: self._buf[:self.draws * self.p1].reshape(self.draws, self.p1))
    pair_r2 = property(lambda self: self._buf[self._off[1]:self._off[1] + self.draws * (self.p1 // 2 + 1)]
                       .reshape(self.draws, self.p1 // 2 + 1))
    gam_sig = property(lambda self: self._buf[self._off[2]:self._off[2] + self.draws])
    gam_tau = property(lambda self: self._buf[self._off[3]:self._off[3] + self.draws])
    progress = property(lambda self: self._int_area()[:1])
    block_done = property(lambda self: self._int_area()[self._ints[0]:self._ints[0] + -(-self.draws // self.BLOCK)])
    lead = property(lambda self: self._int_area()[self._ints[1]:self._ints[1] + self.draws])

    def pointers(self):
        """normals, pair_r2, lead, gam_sig, gam_tau -- the argument order of the C entry points."""
        a, off = self._addr, self._off
        return (a, a + 8 * off[1], a + 8 * off[4] + 4 * self._ints[1], a + 8 * off[2], a + 8 * off[3])

    def progress_pointer(self):
        return self._addr + 8 * self._off[4]

    def rows_pointer(self):
        return self._addr + 8 * self._off[5]

    rows = property(lambda self: self._buf[self._off[5]:self._off[5] + 4 * self.draws].view(np.uint64)
                    .reshape(self.draws, 4))

    def block_done_pointer(self):
        return self._addr + 8 * self._off[4] + 4 * self._ints[0]


def record_noise_tape(tape, astar, atau_star, stream):
    """Fill ``tape`` from the stream on the calling thread."""
    try:
        _check(load().fokl_noise_tape(tape.p1, tape.draws, float(astar), float(atau_star), *stream.args(),
                                      *tape.pointers(), tape.progress_pointer()))
    except BaseException:
        tape.progress[0] = -1
        raise
    return tape


def noise_tape(p1, draws, astar, atau_star, stream):
    return record_noise_tape(NoiseTape(p1, draws), astar, atau_star, stream)


class _StreamCursor(ctypes.Structure):
    _fields_ = [('position', ctypes.c_uint64), ('gauss_source', ctypes.c_uint64), ('has_gauss', ctypes.c_int32)]


class StreamEngine:
    """include/fokl_hip.h: fokl_stream_* -- the random stream as bulk threads + one serial walk, outside a HostPool
    (tests, tools; a fit's engine lives inside its pool).  ``walk`` fills a NoiseTape's rows, ``expand`` turns them into
    the numbers fokl_noise_tape records; the part of the stream a tape covers is held from its walk until ``release``."""

    def __init__(self, stream, bulk_threads=2, prestates=None):
        """prestates: (address, entries) of DeviceChainEngine.prestate_ring() when a device will expand this stream's
        tapes from rows."""
        self._lib = load()
        self._h = None
        self.stream = stream
        h = c_vp(0)
        _check(self._lib.fokl_stream_create(_ptr(stream.key), stream.pos, stream.has_gauss, stream.cache,
                                            int(bulk_threads), prestates[0] if prestates else None,
                                            prestates[1] if prestates else 0, ctypes.byref(h)))
        self._h = h

    def close(self, write_back=True):
        """Stops the bulk threads; the walker's position goes back to ``stream`` as numpy's state tuple."""
        if self._h:
            if write_back:
                _check(self._lib.fokl_stream_state(self._h, *self.stream.args()))
            self._lib.fokl_stream_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close(write_back=False)

    def walk(self, tape, astar, atau_star):
        """One model evaluation's draws: -> the hold that keeps the tape's part of the stream readable."""
        hold = ctypes.c_uint64(0)
        _check(self._lib.fokl_stream_hold(self._h, ctypes.byref(hold)))
        a = tape._addr
        rc = self._lib.fokl_stream_walk(self._h, tape.p1, tape.draws, float(astar), float(atau_star), tape.rows_pointer(),
                                        a + 8 * tape._off[2], a + 8 * tape._off[3], tape.progress_pointer())
        if rc:
            self._lib.fokl_stream_release(self._h, hold)
        _check(rc)
        _check(self._lib.fokl_stream_advance_floor(self._h))
        return hold.value

    def expand(self, tape, astar, atau_star, first=0, last=None):
        ptr = tape.pointers()
        _check(self._lib.fokl_stream_expand(self._h, tape.p1, float(astar), float(atau_star), tape.rows_pointer(),
                                            int(first), tape.draws if last is None else int(last), ptr[0], ptr[1], ptr[2],
                                            ptr[3], ptr[4]))
        return tape

    def release(self, hold):
        _check(self._lib.fokl_stream_release(self._h, ctypes.c_uint64(hold)))

    def tell(self):
        cur = _StreamCursor()
        _check(self._lib.fokl_stream_tell(self._h, ctypes.byref(cur)))
        return cur

    def seek(self, cursor):
        _check(self._lib.fokl_stream_seek(self._h, ctypes.byref(cursor)))

    def numpy_state(self):
        st = LegacyStream(self.stream.as_numpy_state())
        _check(self._lib.fokl_stream_state(self._h, *st.args()))
        return st.as_numpy_state()

    def stats(self):
        b, w, seg, ga, ge = c_dbl(0), c_dbl(0), c_i64(0), c_i64(0), c_i64(0)
        _check(self._lib.fokl_stream_stats(self._h, *[ctypes.byref(x) for x in (b, w, seg, ga, ge)]))
        return dict(bulk_s=b.value, walker_wait_s=w.value, segments=seg.value, gamma_attempts=ga.value,
                    gamma_attempts_exact=ge.value)


def tape_ready(tape):
    """fokl_tape_ready: 1 once the tape is recorded and -- a tape the pool's finish threads work on -- every block is there,
    0 before, -1 if it never will be."""
    return load().fokl_tape_ready(tape.progress_pointer(), tape.draws,
                                  tape.block_done_pointer() if tape.materialised_by_pool else None, tape.BLOCK)


def gibbs_chain_from_tape(lamb, qty, b, btau, dtd, sigsqd0, tausqd0, tape, want_sig_tau=False, follow=False):
    """Replay the chain arithmetic on a tape -- with ``follow=True`` on one that is still being recorded.
    Returns (w, bstar_negative[, sigs, taus])."""
    lamb = np.ascontiguousarray(lamb, dtype=np.float64)
    qty = np.ascontiguousarray(qty, dtype=np.float64)
    p1 = lamb.shape[0]
    if p1 != tape.p1:
        raise ValueError("tape was recorded for a different model size")
    w = np.empty((tape.draws, p1), dtype=np.float64)
    sigs = np.empty(tape.draws) if want_sig_tau else None
    taus = np.empty(tape.draws) if want_sig_tau else None
    flag = ctypes.c_int32(0)
    _check(load().fokl_gibbs_chain_from_tape(_ptr(lamb), _ptr(qty), p1, float(b), float(btau), float(dtd),
                                             float(sigsqd0), float(tausqd0), tape.draws, *tape.pointers(), _ptr(w),
                                             _ptr(sigs), _ptr(taus), ctypes.byref(flag),
                                             tape.progress_pointer() if follow else None))
    if want_sig_tau:
        return w, bool(flag.value), sigs, taus
    return w, bool(flag.value)


def finish_tape_blocks(tape, part=0, parts=1, follow=False):
    """Complete the normals of the tape's blocks part, part + parts, ... in place (fokl_finish_tape_blocks)."""
    ptr = tape.pointers()
    _check(load().fokl_finish_tape_blocks(tape.p1, tape.draws, ptr[0], ptr[1], ptr[2],
                                          tape.progress_pointer() if follow else None, int(part), int(parts),
                                          tape.BLOCK, tape.block_done_pointer()))


def gibbs_chain_from_finished_tape(lamb, qty, b, btau, dtd, sigsqd0, tausqd0, tape, follow=False):
    """The recursion on a tape completed by finish_tape_blocks.  Returns (w, bstar_negative)."""
    lamb = np.ascontiguousarray(lamb, dtype=np.float64)
    qty = np.ascontiguousarray(qty, dtype=np.float64)
    p1 = lamb.shape[0]
    if p1 != tape.p1:
        raise ValueError("tape was recorded for a different model size")
    w = np.empty((tape.draws, p1), dtype=np.float64)
    flag = ctypes.c_int32(0)
    ptr = tape.pointers()
    _check(load().fokl_gibbs_chain_from_finished_tape(_ptr(lamb), _ptr(qty), p1, float(b), float(btau), float(dtd),
                                                      float(sigsqd0), float(tausqd0), tape.draws, ptr[0], ptr[3],
                                                      ptr[4], tape.block_done_pointer() if follow else None,
                                                      tape.BLOCK, _ptr(w), None, None, ctypes.byref(flag)))
    return w, bool(flag.value)


CHAIN_SEGMENTS, CHAIN_WARM = 8, 64      # include/fokl_hip_internal.h: FOKL_CHAIN_SEGMENTS, FOKL_CHAIN_WARM


def gibbs_chain_segments_host(lamb, qty, b, btau, dtd, sigsqd0, tausqd0, tape, follow=False, segments=CHAIN_SEGMENTS,
                              warm=CHAIN_WARM, states=False):
    """gibbs_chain_from_finished_tape with the recursion in verified segments (fokl_gibbs_chain_segments_host).  Returns
    (w, bstar_negative, bad_cut), with states=True also the sigsqd and tausqd of every iteration."""
    lamb = np.ascontiguousarray(lamb, dtype=np.float64)
    qty = np.ascontiguousarray(qty, dtype=np.float64)
    p1 = lamb.shape[0]
    if p1 != tape.p1:
        raise ValueError("tape was recorded for a different model size")
    w = np.empty((tape.draws, p1), dtype=np.float64)
    sigs = np.empty(tape.draws, dtype=np.float64) if states else None
    taus = np.empty(tape.draws, dtype=np.float64) if states else None
    flag, bad_cut = ctypes.c_int32(0), ctypes.c_int32(0)
    ptr = tape.pointers()
    _check(load().fokl_gibbs_chain_segments_host(_ptr(lamb), _ptr(qty), p1, float(b), float(btau), float(dtd),
                                                 float(sigsqd0), float(tausqd0), tape.draws, ptr[0], ptr[3], ptr[4],
                                                 tape.block_done_pointer() if follow else None, tape.BLOCK, _ptr(w),
                                                 _ptr(sigs) if states else None, _ptr(taus) if states else None,
                                                 ctypes.byref(flag), int(segments), int(warm), ctypes.byref(bad_cut)))
    if states:
        return w, bool(flag.value), bool(bad_cut.value), sigs, taus
    return w, bool(flag.value), bool(bad_cut.value)


# ---------------------------------------------------------------------------------------------------------
# host threads of one fit
# ---------------------------------------------------------------------------------------------------------

def _scipy_dsyevd_address():
    """Address of scipy's dsyevd (Fortran ABI, 32-bit integers), or None."""
    try:
        from scipy.linalg import cython_lapack
        capsule = cython_lapack.__pyx_capi__['dsyevd']
        api = ctypes.pythonapi
        api.PyCapsule_GetName.restype = ctypes.c_char_p
        api.PyCapsule_GetName.argtypes = [ctypes.py_object]
        api.PyCapsule_GetPointer.restype = ctypes.c_void_p
        api.PyCapsule_GetPointer.argtypes = [ctypes.py_object, ctypes.c_char_p]
        name = api.PyCapsule_GetName(capsule)
        if name is None or name.count(b'int *') != 6 or b'long' in name:
            return None
        return api.PyCapsule_GetPointer(capsule, name)
    except (ImportError, KeyError):
        return None


def _scipy_dgemm_address():
    """Address of scipy's dgemm (Fortran ABI, 32-bit integers), or None."""
    try:
        from scipy.linalg import cython_blas
        capsule = cython_blas.__pyx_capi__['dgemm']
        api = ctypes.pythonapi
        api.PyCapsule_GetName.restype = ctypes.c_char_p
        api.PyCapsule_GetName.argtypes = [ctypes.py_object]
        api.PyCapsule_GetPointer.restype = ctypes.c_void_p
        api.PyCapsule_GetPointer.argtypes = [ctypes.py_object, ctypes.c_char_p]
        name = api.PyCapsule_GetName(capsule)
        if name is None or name.count(b'int *') != 6 or name.count(b'char *') != 2 or b'long' in name:
            return None
        return api.PyCapsule_GetPointer(capsule, name)
    except (ImportError, KeyError):
        return None


def _scipy_dsyevr_address():
    """Address of the dsyevr that scipy.linalg.eigh itself calls (Fortran ABI, 32-bit integers)."""
    from scipy.linalg import cython_lapack
    capsule = cython_lapack.__pyx_capi__['dsyevr']
    api = ctypes.pythonapi
    api.PyCapsule_GetName.restype = ctypes.c_char_p
    api.PyCapsule_GetName.argtypes = [ctypes.py_object]
    api.PyCapsule_GetPointer.restype = ctypes.c_void_p
    api.PyCapsule_GetPointer.argtypes = [ctypes.py_object, ctypes.c_char_p]
    name = api.PyCapsule_GetName(capsule)
    if name is None or name.count(b'int *') != 11 or b'long' in name:
        raise FoklNativeError(-2, f"unexpected signature of scipy's dsyevr: {name!r}")
    return api.PyCapsule_GetPointer(capsule, name)


class PoolJob:
    """A job on a HostPool.  Keeps the buffers the job reads / writes alive; ``wait()`` may be called repeatedly."""
    __slots__ = ('_h', 'keep', 'result', 'recycle', 'held', 'unresolved', 'ignore_failure', 'co_reader')

    def __init__(self, handle, keep, result=None, tentative=False):
        self._h, self.keep, self.result = handle, keep, result
        self.recycle = None                 # raw buffers the owner of the pool may reuse once the job has run
        self.held = None                    # raw buffer a LATER job will still read: not reusable when this one is done
        self.unresolved = bool(tentative)   # a tentative noise job that has not been given its verdict yet
        self.ignore_failure = False         # a chain started ahead of the decision that it is needed: its tape may go
        self.co_reader = None               # noise job: such a chain, given up, that may still be reading the tape

    def done(self):
        """True once the job has run (its native record is then released, the buffers may go)."""
        if self._h is not None and load().fokl_pool_poll(self._h):
            self.wait()
        return self._h is None

    def resolve(self, commit):
        """Verdict on a tentative noise job (fokl_pool_resolve)."""
        if self.unresolved:
            self.unresolved = False
            _check(load().fokl_pool_resolve(self._h, int(bool(commit))))

    def wait(self):
        if self._h is not None:
            h, self._h = self._h, None
            rc = load().fokl_pool_wait(h)
            if not self.ignore_failure:
                _check(rc)
        return self.result


class SpectralResult:
    """Outputs of fokl_pool_submit_spectral: lamb, Qt (row j = eigenvector j), qty = Q'Xty, betahat, and the residual
    moments (sum r, sum r^2) of y - X betahat formed from the Gram."""
    __slots__ = ('lamb', 'Qt', 'qty', 'betahat', 'moments', '_buf', '_addr')

    @staticmethod
    def doubles(p1):
        return p1 * (p1 + 3) + 2

    def __init__(self, p1, buf=None):
        """buf: an existing float64 buffer of doubles(p1) values holding a result computed elsewhere (another rank)."""
        buf = self._buf = np.empty(p1 * (p1 + 3) + 2, dtype=np.float64) if buf is None else buf
        self._addr = buf.__array_interface__['data'][0]
        self.lamb, self.qty, self.betahat = buf[:p1], buf[p1:2 * p1], buf[2 * p1:3 * p1]
        self.Qt = buf[3 * p1:3 * p1 + p1 * p1].reshape(p1, p1)
        self.moments = buf[3 * p1 + p1 * p1:]

    def pointers(self, p1):
        """lamb_out, qt_out, qty_out, betahat_out, moments_out"""
        a = self._addr
        return (a, a + 24 * p1, a + 8 * p1, a + 16 * p1, a + 8 * p1 * (p1 + 3))


class HostPool:
    """include/fokl_hip.h: fokl_pool_* -- the noise thread (owns ``stream`` until close()), chain threads and
    spectral threads of one fit."""

    def __init__(self, stream, chain_threads=2, finish_threads=2, spectral_threads=3, noise_cpu=-1, bulk_threads=2,
                 prestates=None, device_dgemm=None):
        """prestates: (address, entries) of a pre-state ring (DeviceChainEngine.prestate_ring()) for a device that
        regenerates the stream itself.  device_dgemm: (device, columns) -- the eigen-update's product on that device's matrix
        cores for models of at least that many columns (fokl_device_dgemm), scipy's dgemm below."""
        self._lib = load()
        self.stream = stream
        self._h = None
        h = c_vp(0)
        fn = _scipy_dsyevr_address() if spectral_threads > 0 else None
        self.finish_threads = int(finish_threads)
        _check(self._lib.fokl_pool_create(int(chain_threads), self.finish_threads, int(spectral_threads),
                                          max(1, int(bulk_threads)), int(noise_cpu), c_vp(fn),
                                          *stream.args(), prestates[0] if prestates else None,
                                          prestates[1] if prestates else 0, ctypes.byref(h)))
        self._h = h
        # models of FOKL_EIGH_DC_FROM columns or more (default 80; 0: never): LAPACK's divide-and-conquer driver, which
        # shares dsyevr's tridiagonal reduction and returns its eigenpairs to ~3e-12 in 2/3 of the time (half at 585 columns)
        self.dsyevd_from = 0
        dc_from = int(os.environ.get('FOKL_EIGH_DC_FROM', '80'))
        if spectral_threads > 0 and dc_from > 0 and os.environ.get('FOKL_EIGH_SIGNS', 'canonical') != 'lapack':
            fd = _scipy_dsyevd_address()
            if fd:
                _check(self._lib.fokl_pool_use_dsyevd(self._h, c_vp(fd), dc_from))
                self.dsyevd_from = dc_from
        # the product of the eigen-update (submit_spectral_update; the search core's FOKL_EIGH_UPDATE)
        self.has_dgemm = False
        if spectral_threads > 0:
            fg = _scipy_dgemm_address()
            self.device_dgemm_from = 0
            if fg and device_dgemm is not None:
                entry = c_vp(0)
                if self._lib.fokl_device_dgemm_configure(int(device_dgemm[0]), c_vp(fg), int(device_dgemm[1]),
                                                         ctypes.byref(entry)) == 0 and entry.value:
                    fg, self.device_dgemm_from = entry.value, int(device_dgemm[1])
            if fg:
                _check(self._lib.fokl_pool_use_dgemm(self._h, c_vp(fg)))
                self.has_dgemm = True

    def spectral_affinity(self, cpus):
        cpus = np.ascontiguousarray(sorted(cpus), dtype=np.int32)
        _check(self._lib.fokl_pool_spectral_affinity(self._h, _ptr(cpus), cpus.shape[0]))

    def stream_handle(self):
        """The pool's fokl_stream (for DeviceChainEngine.bind)."""
        return self._lib.fokl_pool_stream(self._h)

    def set_walk_helpers(self, count, cpus=None):
        """fokl_stream_set_helpers on the pool's stream: helper threads for the serial walk (positions + accept tests of the
        blocks the walking thread chases), each on the logical CPU given for it."""
        arr = None
        if cpus is not None:
            arr = np.ascontiguousarray(list(cpus)[:count] + [-1] * max(0, count - len(cpus)), dtype=np.int32)
        _check(self._lib.fokl_stream_set_helpers(c_vp(self.stream_handle()), int(count), _ptr(arr) if arr is not None else None))

    def place_bulk_threads(self, cpus):
        """fokl_stream_place_bulk on the pool's stream: bulk thread i on logical CPU cpus[i % len(cpus)]."""
        arr = np.ascontiguousarray(list(cpus), dtype=np.int32)
        _check(self._lib.fokl_stream_place_bulk(c_vp(self.stream_handle()), _ptr(arr), arr.shape[0]))

    def close(self):
        """Runs everything still queued (each submitted tape advances the stream), then stops the threads."""
        if self._h:
            self._lib.fokl_pool_destroy(self._h)
            self._h = None

    __del__ = close

    def submit_noise(self, tape, astar, atau_star, tentative=False, finish=False):
        """tentative: record ahead of the decision; the job must then get ``resolve(commit)`` (see the header).
        finish: the finish threads complete the tape while it is recorded, before a chain is asked for."""
        h = c_vp(0)
        finish = bool(finish) and self.finish_threads > 0
        _check(self._lib.fokl_pool_submit_noise(self._h, tape.p1, tape.draws, float(astar), float(atau_star),
                                                tape.rows_pointer(), *tape.pointers(), tape.progress_pointer(),
                                                int(bool(tentative)), tape.block_done_pointer(), tape.BLOCK, int(finish),
                                                None, ctypes.byref(h)))
        tape.finishing_requested = finish
        tape.materialised_by_pool = True
        return PoolJob(h, (tape,), tape, tentative)

    def submit_chain(self, lamb, qty, b, btau, dtd, sigsqd0, tausqd0, tape, w_raw=None):
        """Returns a job whose result is (w [draws, p1], bstar_negative int32[1]); w is carved out of the float64 buffer
        w_raw if that is given."""
        p1 = lamb.shape[0]
        if p1 != tape.p1:
            raise ValueError("tape was recorded for a different model size")
        if w_raw is None:
            w = np.empty((tape.draws, p1), dtype=np.float64)
        else:
            w = w_raw[:tape.draws * p1].reshape(tape.draws, p1)
        flag = np.zeros(1, dtype=np.int32)
        h = c_vp(0)
        _check(self._lib.fokl_pool_submit_chain(self._h, _ptr(lamb), _ptr(qty), p1, float(b), float(btau), float(dtd),
                                                float(sigsqd0), float(tausqd0), tape.draws, *tape.pointers(),
                                                tape.progress_pointer(), tape.block_done_pointer(),
                                                tape.BLOCK, int(tape.finishing_requested), _ptr(w), _ptr(flag),
                                                None, None, ctypes.byref(h)))
        return PoolJob(h, (lamb, qty, tape, w, flag), (w, flag))

    def submit_spectral(self, gram, idx, ycol):
        """gram: C-contiguous float64 [L, L]; idx: int32 [p1].  Returns a job whose result is a SpectralResult."""
        p1 = idx.shape[0]
        res = SpectralResult(p1)
        h = c_vp(0)
        _check(self._lib.fokl_pool_submit_spectral(self._h, _ptr(gram), gram.shape[1], _ptr(idx), p1, int(ycol),
                                                   *res.pointers(p1), ctypes.byref(h)))
        return PoolJob(h, (gram, idx, res), res)

    def submit_spectral_update(self, gram, idx, ycol, parent, parent_pos):
        """G2 of gram[idx][:, idx] from the finished SpectralResult ``parent`` of the model that has one more column, at
        position ``parent_pos`` of its column list.  -> (job, updated): updated[0] is 1 when the eigenpairs were derived
        from the parent's, 0 when the model was decomposed afresh after all (once the job has run)."""
        p1 = idx.shape[0]
        res = SpectralResult(p1)
        updated = np.full(1, -1, dtype=np.int32)
        h = c_vp(0)
        _check(self._lib.fokl_pool_submit_spectral_update(self._h, _ptr(gram), gram.shape[1], _ptr(idx), p1, int(ycol),
                                                          _ptr(parent.lamb), _ptr(parent.Qt), int(parent_pos), None,
                                                          *res.pointers(p1), _ptr(updated), ctypes.byref(h)))
        return PoolJob(h, (gram, idx, res, parent, updated), res), updated

    def busy_seconds(self):
        v = [c_dbl(0) for _ in range(4)]
        _check(self._lib.fokl_pool_busy_seconds(self._h, *[ctypes.byref(x) for x in v]))
        w = [c_dbl(0), c_dbl(0)]
        _check(self._lib.fokl_pool_noise_waits(self._h, ctypes.byref(w[0]), ctypes.byref(w[1])))
        b, ww, seg, ga, ge = c_dbl(0), c_dbl(0), c_i64(0), c_i64(0), c_i64(0)
        _check(self._lib.fokl_pool_stream_stats(self._h, *[ctypes.byref(x) for x in (b, ww, seg, ga, ge)]))
        cs = [c_i64(0), c_i64(0)]
        _check(self._lib.fokl_pool_chain_segments(self._h, ctypes.byref(cs[0]), ctypes.byref(cs[1])))
        return dict(noise=v[0].value, chain=v[1].value, finish=v[2].value, spectral=v[3].value,
                    host_chains_segmented=cs[0].value, host_chain_recuts=cs[1].value,
                    noise_queue_wait=w[0].value, noise_verdict_wait=w[1].value, bulk=b.value, walker_wait=ww.value,
                    stream_segments=seg.value, gamma_attempts=ga.value, gamma_attempts_exact=ge.value)


# ---------------------------------------------------------------------------------------------------------
# the native half of a search (include/fokl_hip.h: fokl_search_*)
# ---------------------------------------------------------------------------------------------------------

class _SearchParams(ctypes.Structure):
    _fields_ = [('n', c_i64), ('a', c_dbl), ('b', c_dbl), ('atau', c_dbl), ('btau', c_dbl), ('threshav', c_dbl),
                ('threshstda', c_dbl), ('threshstdb', c_dbl), ('guess_margin', c_dbl), ('draws', c_i32), ('half0', c_i32),
                ('aic', c_i32), ('lookahead', c_i32), ('foresight', c_i32), ('speculation_max', c_i32),
                ('tentative_tapes', c_i32), ('test_rewinds', c_i32), ('device_chain_columns', c_i32),
                ('finish_threads', c_i32), ('flip_guess', c_i32), ('device_rows', c_i32)]


class _OutcomeView(ctypes.Structure):
    _fields_ = [('spectrum', c_vp), ('idx', c_vp), ('ev', c_dbl), ('siglik', c_dbl), ('intercept_scale', c_dbl),
                ('p1', c_i32), ('on_device', c_i32)]


_FORESEE_CB = ctypes.CFUNCTYPE(None, c_vp, ctypes.POINTER(c_i32), c_int)
_IDLE_CB = ctypes.CFUNCTYPE(c_int, c_vp)
_RESIDUAL_CB = ctypes.CFUNCTYPE(c_int, c_vp, ctypes.POINTER(c_i32), c_int, ctypes.POINTER(c_dbl), ctypes.POINTER(c_dbl),
                                ctypes.POINTER(c_dbl))


class _KillTestsArgs(ctypes.Structure):
    _fields_ = [('gram', c_vp), ('columns', c_vp), ('mean_abs', c_vp), ('rel_std', c_vp), ('slots', c_vp), ('best', c_vp),
                ('ahead_keys', c_vp), ('ahead_offsets', c_vp), ('ahead_spectra', c_vp), ('user', c_vp),
                ('foresee', _FORESEE_CB), ('idle_work', _IDLE_CB), ('residual', _RESIDUAL_CB), ('active', c_i32),
                ('proposals', c_i32), ('n_prev', c_i32), ('vm_next', c_i32), ('ahead_count', c_i32)]


class _KillTestsResult(ctypes.Structure):
    _fields_ = [('killed', c_vp), ('best', c_vp), ('evmin', c_dbl), ('killed_count', c_i32), ('best_is_new', c_i32)]


SEARCH_STATS = ('gibbs_calls', 'kill_tests', 'terms_logical', 't_eigh', 't_chain', 'chains_materialised', 'bic_from_gram',
                'tapes_rewound', 'tapes_wasted', 'chains_ahead', 'chains_ahead_unused', 'chains_skipped',
                'spectral_submitted', 'device_chains', 'chains_fetched', 'guessed', 'guess_waits', 'guesses_verified',
                'dchain_kernel_s', 'dchain_timed', 't_resid', 't_kill_loop', 'tapes_materialised', 'rows_chains', 'path_repredicted', 'spectral_device',
                'spectral_updated', 'direct_tests', 'direct_max_rel', 'chains_cancelled', 't_settle',
                'guess_max_dev', 'direct_in_band', 'stats_by_chain_thread')


class NativeSearch:
    """include/fokl_hip.h: fokl_search_* -- the tapes on order, G2 jobs, chains and the kill-test loop of one fit, next to
    its HostPool.  Handles (spectra, tapes, outcomes) are plain integers; engine.NativeOutcome wraps the last kind."""

    def __init__(self, pool, dchain, **params):
        self._lib = load()
        self._h = None
        self._pool, self._dchain = pool, dchain             # keep them alive: the search uses them until close()
        prm = _SearchParams(**params)
        h = c_vp(0)
        _check(self._lib.fokl_search_create(pool._h, dchain._h if dchain is not None else None, ctypes.byref(prm),
                                            ctypes.byref(h)))
        self._h = h
        self.draws = int(params['draws'])

    def close(self):
        if self._h:
            self._lib.fokl_search_destroy(self._h)
            self._h = None

    __del__ = close

    def _checked(self, rc):
        if rc:
            if self._lib.fokl_search_mispredicted(self._h):
                from .host_pipeline import Misprediction
                raise Misprediction(self._lib.fokl_search_error(self._h).decode())
            _check(rc)

    def set_substage(self, term_ids):
        ids = np.ascontiguousarray(term_ids, dtype=np.int64)
        self._checked(self._lib.fokl_search_set_substage(self._h, _ptr(ids), ids.shape[0]))

    def speculate(self, sizes):
        """sizes: [(columns, is_model)] the stream will probably serve next, in order."""
        n = len(sizes)
        cols = np.array([s for s, _ in sizes], dtype=np.int32)
        model = np.array([int(m) for _, m in sizes], dtype=np.int32)
        self._checked(self._lib.fokl_search_speculate(self._h, _ptr(cols), _ptr(model), n))

    def drop_speculation(self):
        self._checked(self._lib.fokl_search_drop_speculation(self._h))

    def bind_spectral(self, engine, max_columns=None, slack=-1.0, lookahead=-1):
        """G2 of models of up to max_columns columns on the device (a DeviceSpectralEngine; None: the pool's threads) when
        requested `slack` kernel durations ahead of need (0: always; < 0: the library's default)."""
        self._spectral_engine = engine                   # kept alive as long as the search
        limit = (engine.max_columns if max_columns is None else int(max_columns)) if engine is not None else 0
        self._checked(self._lib.fokl_search_bind_spectral(self._h, engine._h if engine is not None else None, limit,
                                                          float(slack), int(lookahead)))

    def hold_spectral(self, hold):
        self._checked(self._lib.fokl_search_hold_spectral(self._h, 1 if hold else 0))

    def set_update(self, from_columns, depth, lookahead=0):
        """Kill tests' G2 from the tested-against model's eigenpairs for parents of from_columns columns or more (0: never), at
        most `depth` steps from a fresh decomposition; `lookahead` (0: the search's own): G2 look-ahead while that is on, in
        sub-stages whose model has fewer than 192 columns."""
        self._checked(self._lib.fokl_search_set_update(self._h, int(from_columns), int(depth), int(lookahead)))

    def set_decide(self, mode, tolerance=0.0):
        """Kill tests' BIC decisions: 0 from G2 of every trial model, 1 from the downdated least-squares model of the
        sub-stage, confirmed by the accepted models' eigenpairs to `tolerance` (relative; 0: 1e-9)."""
        self._checked(self._lib.fokl_search_set_decide(self._h, int(mode), float(tolerance)))

    def set_deterministic(self, on=True):
        """Ranks repeating one search side by side: no decision may depend on when a chain's statistics arrive."""
        self._checked(self._lib.fokl_search_set_deterministic(self._h, int(bool(on))))

    def spectral(self, gram, idx, parent=None, parent_pos=-1):
        """parent / parent_pos: a spectrum handle of this search for the model that has one more column, and which of its
        columns this model lacks (G2 may then follow from the parent's eigenpairs, set_update)."""
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        h = c_vp(0)
        if parent is None:
            self._checked(self._lib.fokl_search_spectral(self._h, _ptr(gram), gram.shape[1], _ptr(idx), idx.shape[0],
                                                         ctypes.byref(h)))
        else:
            self._checked(self._lib.fokl_search_spectral_from(self._h, _ptr(gram), gram.shape[1], _ptr(idx), idx.shape[0],
                                                              c_vp(parent), int(parent_pos), ctypes.byref(h)))
        return h.value

    def spectrum_done(self, spectrum):
        return bool(self._lib.fokl_spectrum_done(c_vp(spectrum)))

    def spectrum_view(self, spectrum):
        """-> SpectralResult over the search's own buffer (valid while the spectrum is referenced)."""
        buf, p1 = c_vp(0), c_int(0)
        self._checked(self._lib.fokl_spectrum_wait(self._h, c_vp(spectrum), ctypes.byref(buf), ctypes.byref(p1)))
        n = p1.value
        arr = np.ctypeslib.as_array((ctypes.c_double * SpectralResult.doubles(n)).from_address(buf.value))
        return SpectralResult(n, arr)

    def spectrum_retain(self, spectrum):
        """-> the same handle, holding one more reference (spectrum_release when done with it)."""
        self._checked(self._lib.fokl_spectrum_retain(self._h, c_vp(spectrum)))
        return spectrum

    def spectrum_release(self, spectrum):
        if self._h:
            self._lib.fokl_spectrum_release(self._h, c_vp(spectrum))

    def model_begin(self, gram, idx, given, then):
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        cols = np.array([s for s, _ in then], dtype=np.int32)
        model = np.array([int(m) for _, m in then], dtype=np.int32)
        sp, tape = c_vp(0), c_vp(0)
        self._checked(self._lib.fokl_search_model_begin(self._h, _ptr(gram), gram.shape[1], _ptr(idx), idx.shape[0],
                                                        c_vp(given) if given else None, _ptr(cols), _ptr(model),
                                                        len(then), ctypes.byref(sp), ctypes.byref(tape)))
        return sp.value, tape.value

    def model_commit(self, spectrum, tape, dtd, new_terms=0):
        """new_terms: the model's last `new_terms` active columns are a sub-stage's new terms -- their statistics
        (outcome_new_term_stats) are formed by the chain thread as soon as the chain has run."""
        out = c_vp(0)
        self._checked(self._lib.fokl_search_model_commit(self._h, c_vp(spectrum), c_vp(tape), float(dtd), int(new_terms),
                                                         ctypes.byref(out)))
        return out.value

    def score(self, outcome, s1, s2, n_prev, kill):
        ev = c_dbl(0)
        self._checked(self._lib.fokl_search_score(self._h, c_vp(outcome), float(s1), float(s2), int(n_prev), int(kill),
                                                  ctypes.byref(ev)))
        return ev.value

    def outcome_info(self, outcome):
        view = _OutcomeView()
        self._checked(self._lib.fokl_outcome_info(self._h, c_vp(outcome), ctypes.byref(view)))
        return view

    def outcome_spectrum(self, outcome):
        h = c_vp(0)
        self._checked(self._lib.fokl_outcome_spectrum(self._h, c_vp(outcome), ctypes.byref(h)))
        return h.value

    def outcome_chain_ready(self, outcome):
        return bool(self._lib.fokl_outcome_chain_ready(c_vp(outcome)))

    def outcome_draws(self, outcome, p1):
        w = c_vp(0)
        self._checked(self._lib.fokl_outcome_draws(self._h, c_vp(outcome), ctypes.byref(w)))
        return np.ctypeslib.as_array((ctypes.c_double * (self.draws * p1)).from_address(w.value)).reshape(self.draws, p1)

    def outcome_intercept_scale(self, outcome):
        v = c_dbl(0)
        self._checked(self._lib.fokl_outcome_intercept_scale(self._h, c_vp(outcome), ctypes.byref(v)))
        return v.value

    def outcome_new_term_stats(self, outcome, cols, half0, half1):
        """(|mean beta| over rows half1 .., std over rows half1 .. / |mean over rows half0 ..|) of the model's active columns
        `cols` (FR:1656-1658); waits for the chain."""
        cols = np.ascontiguousarray(cols, dtype=np.int32)
        mean_abs, rel_std = np.empty(cols.shape[0]), np.empty(cols.shape[0])
        self._checked(self._lib.fokl_outcome_new_term_stats(self._h, c_vp(outcome), _ptr(cols), cols.shape[0], int(half0),
                                                            int(half1), _ptr(mean_abs), _ptr(rel_std)))
        return mean_abs, rel_std

    def outcome_release(self, outcome):
        if self._h:
            self._lib.fokl_outcome_release(self._h, c_vp(outcome))

    def outcome_drop(self, outcome):
        if self._h:
            self._lib.fokl_outcome_drop(self._h, c_vp(outcome))

    def verify(self, block=False):
        self._checked(self._lib.fokl_search_verify(self._h, int(bool(block))))

    def register_forecast(self, key, spectrum, dtd):
        key = np.ascontiguousarray(key, dtype=np.int32)
        self._checked(self._lib.fokl_search_register_forecast(self._h, _ptr(key), key.shape[0], c_vp(spectrum), float(dtd)))

    def clear_forecasts(self):
        self._lib.fokl_search_clear_forecasts(self._h)

    def likely_first_tests(self, spectrum, n_new, siglik=None):
        """-> [(active column, probably accepted)] in testing order (fokl_search_likely_first_tests)."""
        out = np.empty(max(1, int(n_new)), dtype=np.int32)
        acc = np.zeros(max(1, int(n_new)), dtype=np.int32)
        count = c_int(0)
        self._checked(self._lib.fokl_search_likely_first_tests(self._h, c_vp(spectrum), int(n_new),
                                                               float('nan') if siglik is None else float(siglik),
                                                               _ptr(out), _ptr(acc), ctypes.byref(count)))
        return [(int(c), bool(a)) for c, a in zip(out[:count.value], acc[:count.value])]

    def stats(self):
        v = np.zeros(len(SEARCH_STATS) + 8)
        n = self._lib.fokl_search_stats(self._h, _ptr(v), v.shape[0])
        if n != len(SEARCH_STATS):
            raise FoklNativeError(-3, "fokl_search_stats: the library's counters do not match SEARCH_STATS")
        return dict(zip(SEARCH_STATS, v[:n].tolist()))

    def trace(self):
        n = self._lib.fokl_search_trace(self._h, None, 0)
        rec = np.zeros((max(1, n), 5))
        self._lib.fokl_search_trace(self._h, _ptr(rec), n)
        return TraceRecords(rec[:n])

    def kill_tests(self, gram, columns, mean_abs, rel_std, slots, best, n_prev, vm_next, ahead, foresee=None,
                   idle_work=None, residual=None):
        """fokl_search_kill_tests.  ahead: {frozenset of active columns: spectrum handle}; the callbacks are Python
        callables -- foresee(list of killed columns), idle_work(), residual(idx, betahat) -> (s1, s2) -- whose exceptions
        are re-raised here after the native loop has returned.  -> (killed columns, evmin, best handle, best_is_new)."""
        A = int(gram.shape[0]) - 1
        vm = int(columns.shape[0])
        columns = np.ascontiguousarray(columns, dtype=np.int32)
        mean_abs = np.ascontiguousarray(mean_abs, dtype=np.float64)
        rel_std = np.ascontiguousarray(rel_std, dtype=np.float64)
        slots = np.ascontiguousarray(slots, dtype=np.int32)
        keys, offsets, handles = [], [0], []
        for key, h in ahead.items():
            keys.extend(sorted(key))
            offsets.append(len(keys))
            handles.append(h)
        keys = np.array(keys if keys else [0], dtype=np.int32)
        offsets = np.array(offsets, dtype=np.int32)
        handle_arr = (c_vp * max(1, len(handles)))(*handles)
        raised = []

        def guard(fn, *args):
            try:
                return fn(*args)
            except BaseException as exc:                     # noqa: B902 -- carried over the native frame
                raised.append(exc)
                return None

        def cb_foresee(_user, killed, count):
            if not raised:
                guard(foresee, [int(killed[i]) for i in range(count)])

        def cb_idle(_user):
            if not raised:
                guard(idle_work)
            return -3 if raised else 0

        def cb_residual(_user, idx, p1, betahat, s1, s2):
            if not raised:
                got = guard(residual, np.array([idx[i] for i in range(p1)], dtype=np.int32),
                            np.array([betahat[i] for i in range(p1)]))
                if got is not None:
                    s1[0], s2[0] = float(got[0]), float(got[1])
            return -3 if raised else 0

        killed = np.zeros(max(1, vm), dtype=np.int32)
        args = _KillTestsArgs(
            gram=_ptr(gram), columns=_ptr(columns), mean_abs=_ptr(mean_abs), rel_std=_ptr(rel_std),
            slots=_ptr(slots), best=best, ahead_keys=_ptr(keys), ahead_offsets=_ptr(offsets),
            ahead_spectra=ctypes.cast(handle_arr, c_vp).value, user=None,
            foresee=_FORESEE_CB(cb_foresee) if foresee is not None else _FORESEE_CB(),
            idle_work=_IDLE_CB(cb_idle) if idle_work is not None else _IDLE_CB(),
            residual=_RESIDUAL_CB(cb_residual) if residual is not None else _RESIDUAL_CB(),
            active=A, proposals=vm, n_prev=int(n_prev), vm_next=-1 if vm_next is None else int(vm_next),
            ahead_count=len(handles))
        res = _KillTestsResult(killed=_ptr(killed))
        rc = self._lib.fokl_search_kill_tests(self._h, ctypes.byref(args), ctypes.byref(res))
        if raised:
            raise raised[0]
        self._checked(rc)
        return [int(c) for c in killed[:res.killed_count]], float(res.evmin), res.best, bool(res.best_is_new)


# ---------------------------------------------------------------------------------------------------------
# G3 on the device
# ---------------------------------------------------------------------------------------------------------

class _PinnedBlock:
    """Owner of one fokl_host_alloc allocation.  When the last array view of it goes the block returns to a free list
    of its size (page-locking and unlocking cost milliseconds; tapes come and go by the hundred per fit)."""
    __slots__ = ('ptr', 'nbytes')
    FREE = {}                                                     # nbytes -> [addresses]
    KEEP_BYTES = int(float(os.environ.get('FOKL_PINNED_POOL_MB', '1024')) * (1 << 20))
    kept = 0

    def __init__(self, nbytes):
        spare = _PinnedBlock.FREE.get(nbytes)
        if spare:
            self.ptr = spare.pop()
            _PinnedBlock.kept -= nbytes
        else:
            ptr = c_vp(0)
            _check(load().fokl_host_alloc(ctypes.c_size_t(nbytes), ctypes.byref(ptr)))
            self.ptr = ptr.value
        self.nbytes = nbytes

    def __del__(self):
        try:
            if self.ptr:
                if _PinnedBlock.kept + self.nbytes <= _PinnedBlock.KEEP_BYTES:
                    _PinnedBlock.FREE.setdefault(self.nbytes, []).append(self.ptr)
                    _PinnedBlock.kept += self.nbytes
                else:
                    load().fokl_host_free(c_vp(self.ptr))
        except Exception:                                          # interpreter shutdown: the driver reclaims it anyway
            pass
        self.ptr = None


def pinned_empty(doubles):
    """A float64 array of ``doubles`` elements in page-locked host memory (tapes that the device chains read in place)."""
    block = _PinnedBlock(int(doubles) * 8)
    raw = (ctypes.c_double * int(doubles)).from_address(block.ptr)
    raw._fokl_owner = block                                       # the ctypes array is the ndarray's base: keeps the block
    return np.ctypeslib.as_array(raw)


class DeviceChainJob:
    """One chain on a DeviceChainEngine (include/fokl_hip.h: fokl_dchain_*).  ``wait()`` -> (mean of w over the rows
    from ``stat_first`` on, bstar-negative flag); ``fetch_w()`` -> the draws in the eigenbasis [draws, p1];
    ``release()`` frees the device slot (idempotent).  Keeps the host buffers the job reads alive.
    Completion is read from the job's statistics area in page-locked host memory (the kernel stores the ticket there
    last): ``done()`` is a memory load, not a call into the runtime."""
    __slots__ = ('_engine', '_ticket', 'p1', 'draws', 'keep', 'recycle', '_stats', 'ignore_failure', '_area', '_flag',
                 '_mark', '_misses')
    unresolved = False                  # PoolJob's interface: only tentative noise jobs wait for a verdict

    def __init__(self, engine, ticket, p1, draws, keep, stats_address=None):
        self._engine, self._ticket, self.p1, self.draws, self.keep = engine, ticket, p1, draws, keep
        self.recycle = None
        self._stats = None
        self.ignore_failure = False
        self._area = self._flag = None
        self._mark = float(ticket) if ticket is not None else 0.0
        self._misses = 0
        if stats_address:
            self._area = np.ctypeslib.as_array((ctypes.c_double * (7 + p1)).from_address(stats_address))
            self._flag = ctypes.c_double.from_address(stats_address + 8 * (4 + p1))

    def resolve(self, commit):
        pass

    def _ran(self):
        return self._flag is not None and self._flag.value == self._mark

    def done(self):
        """True once the device is through with the job's host buffers (the chain has run, or the job has failed)."""
        if self._ticket is None or self._stats is not None or self._ran():
            return True
        if self._flag is not None:
            # a failed job never sets the flag: the engine is asked now and then (it knows a failed job: poll reports it as
            # finished, wait() / release() report the error), so that such a job does not hold its buffers for good
            self._misses += 1
            if self._misses % 64:
                return False
        return bool(self._engine._lib.fokl_dchain_poll(self._engine._h, self._ticket))

    def wait(self):
        if self._stats is None:
            if self._ticket is None:
                raise RuntimeError("device chain: released before anybody read its statistics")
            if self._ran():
                self._stats = np.array(self._area[:4 + self.p1])
            else:
                buf = np.empty(4 + self.p1, dtype=np.float64)
                _check(self._engine._lib.fokl_dchain_wait(self._engine._h, self._ticket, _ptr(buf)))
                self._stats = buf
        return self._stats[4:], np.array([int(self._stats[0])], dtype=np.int32)

    @property
    def kernel_seconds(self):
        """How long the chain's wavefront ran, by the kernel's own clock (0.0 if not known)."""
        if self._area is not None and self._ran():
            return float(self._area[5 + self.p1])
        return 0.0

    @property
    def rows_averaged(self):
        """How many rows (from ``stat_first`` on) the mean of w was formed over."""
        self.wait()
        return int(self._stats[3])

    @property
    def bad_cut(self):
        """True when the segmented recursion found the chain not to forget its state within a warm-up and ran it again in
        one piece (read in place: before ``release``)."""
        self.wait()
        if self._area is None:
            raise RuntimeError("device chain: released, its statistics area belongs to another chain")
        return bool(self._area[6 + self.p1] != 0.0)

    @property
    def last_state(self):
        """(sigma^2, tau^2) after the last iteration."""
        self.wait()
        return float(self._stats[1]), float(self._stats[2])

    def fetch_w(self, out=None):
        w = np.empty((self.draws, self.p1), dtype=np.float64) if out is None else out
        _check(self._engine._lib.fokl_dchain_fetch_w(self._engine._h, self._ticket, _ptr(w)))
        return w

    def try_release(self):
        """release() if that takes no waiting.  -> True when the slot is free."""
        if self._ticket is None or not self._engine._h:
            return True
        if self._flag is not None and not self._ran() and self._stats is None:
            return False
        if self._engine._lib.fokl_dchain_try_release(self._engine._h, self._ticket):
            self._ticket, self.keep, self._area, self._flag = None, None, None, None
            return True
        return False

    def release(self):
        if self._ticket is not None and self._engine._h:
            self._engine._lib.fokl_dchain_release(self._engine._h, self._ticket)
        self._ticket = None
        self.keep = self._area = self._flag = None


class DeviceChainEngine:
    """include/fokl_hip.h: fokl_dchain_* -- finishing of the polar normals and the Gibbs recursion on the GPU."""
    max_columns = 768                   # one wavefront per chain, up to 12 eigen-directions per lane

    def __init__(self, device=0, slots=96):
        self._lib = load()
        self._h = None
        h = c_vp(0)
        _check(self._lib.fokl_dchain_create(int(device), int(slots), ctypes.byref(h)))
        self._h = h
        self.device = int(device)

    def close(self):
        if self._h:
            self._lib.fokl_dchain_destroy(self._h)
            self._h = None

    __del__ = close

    def submit(self, lamb, qty, b, btau, dtd, sigsqd0, tausqd0, tape, stat_first=0, follow=True):
        """Queue the chain of ``tape`` (a NoiseTape, possibly still on record: ``follow``) for the model (lamb, qty)."""
        lamb = np.ascontiguousarray(lamb, dtype=np.float64)
        qty = np.ascontiguousarray(qty, dtype=np.float64)
        p1 = lamb.shape[0]
        if p1 != tape.p1:
            raise ValueError("tape was recorded for a different model size")
        ptr = tape.pointers()
        finished = bool(tape.finishing_requested)
        ticket, area = c_i64(0), c_vp(0)
        _check(self._lib.fokl_dchain_submit(self._h, p1, tape.draws, _ptr(lamb), _ptr(qty), float(b), float(btau),
                                            float(dtd), float(sigsqd0), float(tausqd0), ptr[0], ptr[2], ptr[3], ptr[4],
                                            tape.progress_pointer() if follow else None,
                                            tape.block_done_pointer() if finished or tape.materialised_by_pool else None,
                                            tape.BLOCK, int(finished),
                                            int(stat_first), ctypes.byref(ticket), ctypes.byref(area)))
        return DeviceChainJob(self, ticket.value, p1, tape.draws, (tape,), area.value)

    def prestate_ring(self):
        """(address, entries) of the page-locked ring a stream's bulk threads leave its pre-states in: hand it to the
        HostPool / StreamEngine whose tapes this engine will expand from rows, then ``bind`` that stream."""
        ring, entries = c_vp(0), c_int(0)
        _check(self._lib.fokl_dchain_prestate_ring(self._h, ctypes.byref(ring), ctypes.byref(entries)))
        return ring.value, entries.value

    def bind(self, stream_handle):
        _check(self._lib.fokl_dchain_bind_stream(self._h, stream_handle))

    def submit_rows(self, lamb, qty, b, btau, dtd, sigsqd0, tausqd0, astar, atau_star, tape, span, stat_first=0):
        """The chain of a tape that exists as rows (``tape.rows``, its gamma arrays and progress word in page-locked
        memory); span: uint64 [2] as fokl_pool_submit_noise fills it (position held from, position behind the tape)."""
        lamb = np.ascontiguousarray(lamb, dtype=np.float64)
        qty = np.ascontiguousarray(qty, dtype=np.float64)
        p1 = lamb.shape[0]
        ptr = tape.pointers()
        ticket, area = c_i64(0), c_vp(0)
        _check(self._lib.fokl_dchain_submit_rows(self._h, p1, tape.draws, _ptr(lamb), _ptr(qty), float(b), float(btau),
                                                 float(dtd), float(sigsqd0), float(tausqd0), float(astar), float(atau_star),
                                                 tape.rows_pointer(), ptr[3], ptr[4], tape.progress_pointer(), _ptr(span),
                                                 int(stat_first), ctypes.byref(ticket), ctypes.byref(area)))
        return DeviceChainJob(self, ticket.value, p1, tape.draws, (tape, span), area.value)

    def stream_stats(self):
        seg, rows = c_i64(0), c_i64(0)
        _check(self._lib.fokl_dchain_stream_stats(self._h, ctypes.byref(seg), ctypes.byref(rows)))
        return dict(segments_made=seg.value, rows_jobs=rows.value)

    def flush(self):
        """Issue what is queued now (the caller knows that nothing more is coming for a while)."""
        _check(self._lib.fokl_dchain_flush(self._h))

    def stats(self):
        busy, issued, launches, staged = c_dbl(0), c_i64(0), c_i64(0), c_i64(0)
        _check(self._lib.fokl_dchain_stats(self._h, ctypes.byref(busy), ctypes.byref(issued), ctypes.byref(launches),
                                           ctypes.byref(staged)))
        recuts = c_i64(0)
        _check(self._lib.fokl_dchain_recuts(self._h, ctypes.byref(recuts)))
        return dict(dispatch_s=busy.value, issued=issued.value, launches=launches.value, staged=staged.value,
                    recuts=recuts.value)


class DeviceSpectralJob:
    """One eigen-decomposition on the device; the arrays are views of the engine's page-locked result area (valid until
    ``release``)."""

    def __init__(self, engine, ticket, result, p1):
        self.engine, self.ticket, self.p1 = engine, int(ticket), int(p1)
        n = self.p1
        area = (ctypes.c_double * (n * n + 3 * n + 7)).from_address(result)
        self._area = np.frombuffer(area, dtype=np.float64)
        self._released = False

    def done(self):
        rc = self.engine._lib.fokl_dspectral_poll(self.engine._h, self.ticket)
        if rc < 0:
            _check(-rc)
        return rc == 1

    def wait(self):
        """-> (lamb, Qt, qty, betahat, moments) like HostPool's spectral job."""
        _check(self.engine._lib.fokl_dspectral_wait(self.engine._h, self.ticket))
        n, a = self.p1, self._area
        return a[:n], a[3 * n:3 * n + n * n].reshape(n, n), a[n:2 * n], a[2 * n:3 * n], a[3 * n + n * n:3 * n + n * n + 2]

    def info(self):
        """-> dict(sweeps, rotations, seconds on the device) of a job that has run."""
        a = self._area[3 * self.p1 + self.p1 * self.p1 + 2:]
        return dict(sweeps=int(a[0]), rotations=int(a[1]), seconds=float(a[2]), not_converged=bool(a[3]))

    def release(self):
        if not self._released and self.engine._h:
            self._released = True
            _check(self.engine._lib.fokl_dspectral_release(self.engine._h, self.ticket))


class DeviceSpectralEngine:
    """include/fokl_hip.h: fokl_dspectral_* -- G2 (eigh of XtX sub-blocks, Q'Xty, betahat, residual moments) on the GPU."""

    def __init__(self, device=0):
        self._lib = load()
        self._h = None
        h = c_vp(0)
        _check(self._lib.fokl_dspectral_create(int(device), ctypes.byref(h)))
        self._h = h
        self.device = int(device)
        self.max_columns = int(self._lib.fokl_dspectral_max_columns())

    def close(self):
        if self._h:
            self._lib.fokl_dspectral_destroy(self._h)
            self._h = None

    __del__ = close

    def set_signs(self, canonical=True):
        _check(self._lib.fokl_dspectral_set_signs(self._h, 1 if canonical else 0))

    def submit(self, gram, idx, launch=True):
        """Queue the decomposition of gram[idx][:, idx] (gram: [(A + 1), (A + 1)], ones column first, y last)."""
        gram = np.ascontiguousarray(gram, dtype=np.float64)
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        ticket, result = c_i64(0), c_vp(0)
        _check(self._lib.fokl_dspectral_submit(self._h, _ptr(gram), int(gram.shape[0]), _ptr(idx), int(idx.size),
                                               int(gram.shape[0]) - 1, 1 if launch else 0, ctypes.byref(ticket),
                                               ctypes.byref(result)))
        return DeviceSpectralJob(self, ticket.value, result.value, idx.size)

    def flush(self):
        _check(self._lib.fokl_dspectral_flush(self._h))

    def stats(self):
        submitted, launches = c_i64(0), c_i64(0)
        _check(self._lib.fokl_dspectral_stats(self._h, ctypes.byref(submitted), ctypes.byref(launches)))
        return dict(submitted=submitted.value, launches=launches.value)


def gibbs_chain_device(engine, lamb, qty, b, btau, dtd, sigsqd0, tausqd0, tape, stat_first=0):
    """One chain on the device, start to finish: -> (w [draws, p1], mean of w from row stat_first, bstar-negative)."""
    job = engine.submit(lamb, qty, b, btau, dtd, sigsqd0, tausqd0, tape, stat_first, follow=False)
    try:
        mean_w, flag = job.wait()
        return job.fetch_w(), np.array(mean_w), bool(flag[0])
    finally:
        job.release()


# ---------------------------------------------------------------------------------------------------------
# device context
# ---------------------------------------------------------------------------------------------------------

_OPS_SIGS = (('reserve_slots', [c_vp, c_int]),
             ('build_terms', [c_vp, c_vp, c_int, c_vp]),
             ('gram', [c_vp, c_vp, c_int, c_vp, c_int, c_vp, c_int, c_int]),
             ('gram_launch', [c_vp, c_vp, c_int, c_vp, c_int, c_int]),
             ('gram_fetch', [c_vp, c_vp, c_i64]),
             ('gram_ready', [c_vp]),
             ('bic_resid', [c_vp, c_vp, c_int, c_vp, c_vp, c_int]),
             ('bic_resid_launch', [c_vp, c_vp, c_int, c_vp]),
             ('bic_resid_fetch', [c_vp, c_vp, c_int]),
             ('bic_resid_terms_launch', [c_vp, c_vp, c_int, c_vp]))
_OPS_TYPES = {name: ctypes.CFUNCTYPE(c_int, *args) for name, args in _OPS_SIGS}


class _BackendOps(ctypes.Structure):
    _fields_ = [('ctx', c_vp)] + [(name, c_vp) for name, _ in _OPS_SIGS] + [('kernel_id', c_i32)]


class _RunParams(ctypes.Structure):
    _fields_ = [(name, c_i32) for name in (
        'm', 'n_phis', 'way3', 'tolerance', 'gimmie', 'draws', 'half0', 'lookahead', 'lookahead_native', 'foresight',
        'speculate_across', 'forecast_early', 'forecast_polls', 'matrix_free', 'update_from', 'update_depth',
        'update_lookahead', 'head_start', 'slot_capacity')]


RUN_STATS = ('terms_physical', 'substages', 'forecasts_used', 'forecasts_early', 'resid_matrix_free', 't_resid',
             'phase_prepare', 'phase_model', 'phase_statistics', 'phase_tests', 'phase_wrap_up')
# fokl_run_order's columns: when (monotonic clock, seconds) each step of a sub-stage's model went out; None: not there
RUN_ORDER = ('k1_ahead', 'g2_wait_begun', 'g2_arrived', 'chain_submitted', 'orders_placed', 'k3_launched', 'ahead_gram_launched')


def backend_ops(backend, kernel_id):
    """include/fokl_hip_internal.h fokl_backend_ops for a search backend -> (struct, what must stay alive with it).
    A backend on a DeviceContext hands over the library's own entry points (nothing of the loop passes through Python); any
    other object with HipBackend's methods (the checker backend of the CPU tests) is reached through callbacks."""
    lib = load()
    ops = _BackendOps()
    ops.kernel_id = int(kernel_id)
    ctx = getattr(backend, 'ctx', None)
    if isinstance(ctx, DeviceContext):
        ops.ctx = ctx._h
        for name, _ in _OPS_SIGS:
            setattr(ops, name, ctypes.cast(getattr(lib, 'fokl_' + name), c_vp).value)
        return ops, (ctx,)
    pending, raised = {}, []

    def arr(ptr, count, ctype, dtype):
        return np.array(np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(ctype * count)).contents), dtype=dtype)

    def guard(fn):
        def call(*args):
            try:
                fn(*args)
                return 0
            except BaseException as exc:                     # noqa: B902 -- carried over the native frame
                raised.append(exc)
                return -3
        return call

    def out(ptr, values):
        values = np.ascontiguousarray(values, dtype=np.float64).reshape(-1)
        ctypes.memmove(ptr, values.ctypes.data, values.nbytes)

    def reserve_slots(_c, n):
        backend.reserve_slots(int(n))

    def build_terms(_c, terms, T, slots):
        sl = arr(slots, T, ctypes.c_int32, np.int32)
        m = pending['m']
        backend.build_terms(arr(terms, T * m, ctypes.c_int32, np.int32).reshape(T, m), [int(v) for v in sl])

    def gram(_c, rows, nr, cols, nc, dst, _path, allreduce):
        out(dst, backend.gram([int(v) for v in arr(rows, nr, ctypes.c_int32, np.int32)],
                              [int(v) for v in arr(cols, nc, ctypes.c_int32, np.int32)], bool(allreduce)))

    def gram_launch(_c, rows, nr, cols, nc, allreduce):
        pending['gram'] = backend.gram([int(v) for v in arr(rows, nr, ctypes.c_int32, np.int32)],
                                       [int(v) for v in arr(cols, nc, ctypes.c_int32, np.int32)], bool(allreduce))

    def gram_fetch(_c, dst, count):
        block = pending.pop('gram')
        assert block.size == count
        out(dst, block)

    def bic_resid(_c, slots, nc, betahat, dst, allreduce):
        out(dst, backend.bic_resid([int(v) for v in arr(slots, nc, ctypes.c_int32, np.int32)],
                                   arr(betahat, nc, ctypes.c_double, np.float64), bool(allreduce)))

    def bic_resid_launch(_c, slots, nc, betahat):
        pending['resid'] = backend.bic_resid([int(v) for v in arr(slots, nc, ctypes.c_int32, np.int32)],
                                             arr(betahat, nc, ctypes.c_double, np.float64), False)

    def bic_resid_fetch(_c, dst, _allreduce):
        out(dst, pending.pop('resid'))

    def bic_resid_terms_launch(_c, terms, n_terms, betahat):
        m = pending['m']
        pending['resid'] = backend.bic_resid_terms_launch(arr(terms, n_terms * m, ctypes.c_int32, np.int32).reshape(n_terms, m),
                                                          arr(betahat, n_terms + 1, ctypes.c_double, np.float64))

    table = dict(reserve_slots=reserve_slots, build_terms=build_terms, gram=gram, gram_launch=gram_launch,
                 gram_fetch=gram_fetch, bic_resid=bic_resid, bic_resid_launch=bic_resid_launch,
                 bic_resid_fetch=bic_resid_fetch)
    if hasattr(backend, 'bic_resid_terms_launch'):          # (a stand-in with a matrix-free pass: -> the moments, fetched as above)
        table['bic_resid_terms_launch'] = bic_resid_terms_launch
    keep = [pending, raised]
    for name, fn in table.items():
        cb = _OPS_TYPES[name](guard(fn))
        keep.append(cb)
        setattr(ops, name, ctypes.cast(cb, c_vp).value)
    return ops, tuple(keep)


class NativeRun:
    """include/fokl_hip_internal.h: fokl_run_* -- the sub-stage loop of a fit (csrc/fokl_run.cpp) on a NativeSearch.
    Created BEFORE the pool (its head start puts the first sub-stage's columns and Gram block under way)."""

    def __init__(self, backend, kernel_id, **params):
        self._lib = load()
        self._h = None
        self._ops, self._keep = backend_ops(backend, kernel_id)
        if isinstance(self._keep[0], dict):
            self._keep[0]['m'] = int(params['m'])
        self._prm = _RunParams(**{k: int(v) for k, v in params.items()})
        self.m = int(params['m'])
        h = c_vp(0)
        _check(self._lib.fokl_run_create(ctypes.byref(self._ops), ctypes.byref(self._prm), ctypes.byref(h)))
        self._h = h
        self._reraise()

    def _reraise(self):
        raised = self._keep[1] if isinstance(self._keep[0], dict) else None
        if raised:
            exc = raised[0]
            del raised[:]
            raise exc

    def set_update(self, from_columns, depth, lookahead):
        _check(self._lib.fokl_run_set_update(self._h, int(from_columns), int(depth), int(lookahead)))

    def search(self, native_search):
        """The loop.  Raises what a backend callback raised, or FoklNativeError with the search's / the run's message."""
        rc = self._lib.fokl_run_search(self._h, native_search._h)
        self._reraise()
        if rc != 0:
            native_search._checked(rc)
        return self

    def result(self):
        """-> (mtx [rows, m] float64, evs, per sub-stage (mean_abs, rel_std), handle of the returned model, handle of the
        last sub-stage's survivor, stats)"""
        rows, n_evs, subs = c_i32(0), c_i32(0), c_i32(0)
        best, last = c_vp(0), c_vp(0)
        _check(self._lib.fokl_run_result(self._h, ctypes.byref(rows), ctypes.byref(n_evs), ctypes.byref(subs),
                                         ctypes.byref(best), ctypes.byref(last)))
        mtx = np.zeros((max(rows.value, 0), self.m), dtype=np.int32)
        evs = np.zeros(n_evs.value)
        sizes = np.zeros(max(subs.value, 1), dtype=np.int32)
        stats = np.zeros(16)
        total = self._lib.fokl_run_arrays(self._h, _ptr(mtx) if mtx.size else None, _ptr(evs) if evs.size else None,
                                          _ptr(sizes), None, None, _ptr(stats))
        mean_abs, rel_std = np.zeros(max(total, 1)), np.zeros(max(total, 1))
        self._lib.fokl_run_arrays(self._h, None, None, None, _ptr(mean_abs), _ptr(rel_std), None)
        per, at = [], 0
        for size in sizes[:subs.value]:
            per.append(dict(mean_abs=mean_abs[at:at + size].copy(), rel_std=rel_std[at:at + size].copy()))
            at += int(size)
        st = dict(zip(RUN_STATS, stats[:len(RUN_STATS)]))
        order = np.full((max(self._lib.fokl_run_order(self._h, None, 0), 1), len(RUN_ORDER)), np.nan)
        rows = self._lib.fokl_run_order(self._h, _ptr(order), order.shape[0])
        st['substage_order'] = [{k: (None if np.isnan(v) else float(v)) for k, v in zip(RUN_ORDER, row)} for row in order[:rows]]
        return (mtx.astype(np.float64), evs, per, best.value, last.value, st)

    def close(self):
        if self._h is not None and self._h:
            self._lib.fokl_run_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _FirstTrialStruct(ctypes.Structure):
    """fokl_control_first_trial (include/fokl_hip_internal.h)"""
    _fields_ = [(name, ctypes.c_void_p) for name in ('trial', 'slope', 'moved', 'pooled', 'ft', 'ft_sums', 'phi_t', 'a_t', 'z',
                                                      'status', 'descent')]


class _SystemStruct(ctypes.Structure):
    """fokl_system (include/fokl_hip_internal.h)"""
    _fields_ = [('n_members', c_int), ('n_states', c_int), ('n_steps', c_i64), ('h', c_dbl), ('n_forcing_cols', c_int),
                ('forcing', c_vp), ('n_norm_forcing', c_int), ('n_norm', c_int), ('norm_src', c_vp), ('norm_lo', c_vp),
                ('norm_span', c_vp), ('n_forcing_factors', c_int), ('n_factors', c_int), ('fac_norm', c_vp), ('fac_kind', c_vp),
                ('fac_row', c_vp), ('fac_degree', c_vp), ('n_spline_rows', c_int), ('spline_table', c_vp), ('n_bern_rows', c_int),
                ('bern_table', c_vp), ('n_entries', c_int), ('entries', c_vp), ('entry_begin', c_vp), ('entry_count', c_vp),
                ('constant', c_vp), ('n_coef', c_int), ('coef', c_vp), ('y0', c_vp), ('box', c_vp)]


class _ControlProblemStruct(ctypes.Structure):
    """fokl_control_problem (include/fokl_hip_internal.h)"""
    _fields_ = [('n_controls', c_int), ('n_segments', c_int), ('seg_first', c_vp), ('norm_control', c_vp), ('ctl_lo', c_vp),
                ('ctl_width', c_vp), ('ref', c_vp), ('track_weight', c_vp), ('terminal_weight', c_vp), ('limit_lo', c_vp),
                ('limit_hi', c_vp), ('limit_weight', c_dbl), ('move_weight', c_vp), ('previous', c_vp), ('has_previous', c_int),
                ('n_starts', c_int), ('z0', c_vp), ('max_iter', c_int), ('tol', c_dbl)]


class _CalibrateProblemStruct(ctypes.Structure):
    """fokl_calibrate_problem (include/fokl_hip_internal.h)"""
    _fields_ = [('n_unknown', c_int), ('unknown_src', c_vp), ('norm_param', c_vp), ('lo', c_vp), ('hi', c_vp), ('prior_mean', c_vp),
                ('prior_prec', c_vp), ('starts', c_vp), ('n_observed', c_int), ('obs_state', c_vp), ('obs_hp', c_vp), ('n_obs', c_int),
                ('obs_row', c_vp), ('data', c_vp), ('draw_ids', c_vp), ('burnin', c_int), ('draws_kept', c_int), ('thin', c_int),
                ('jump_every', c_int), ('seed', ctypes.c_uint32)]


_i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
_f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64)


def _system_struct(p, who, coef_by_draw):
    """The fokl_system of a prepared ``p`` -> (struct, the arrays it points into: the caller keeps them referenced until the
    call has returned).  ``coef_by_draw``: coef goes as [E, n_coef] (assimilate, control), otherwise as [n_coef, E]."""
    K, E, steps = int(p['K']), int(p['E']), int(p['n_steps'])
    a = dict(forcing=_f64(p['forcing']), norm_src=_i32(p['norm_src']), norm_lo=_f64(p['norm_lo']), norm_span=_f64(p['norm_span']),
             fac_norm=_i32(p['fac_norm']), fac_kind=_i32(p['fac_kind']), fac_row=_i32(p['fac_row']), fac_degree=_i32(p['fac_degree']),
             spline_table=_f64(p['spline_table']), bern_table=_f64(p['bern_table']), entries=_i32(p['entries']).reshape(-1, 4),
             entry_begin=_i32(p['entry_begin']), entry_count=_i32(p['entry_count']), constant=_i32(p['constant']),
             coef=_f64(np.asarray(p['coef']).T if coef_by_draw else p['coef']), y0=_f64(p['y0']), box=_f64(p['box']))
    coef, forcing, bern = a['coef'], a['forcing'], a['bern_table']
    if coef.ndim != 2 or coef.shape[0 if coef_by_draw else 1] != E or a['y0'].shape != (K, E) or a['box'].shape != (K, 2) or \
            a['entry_begin'].shape != (K,) or a['entry_count'].shape != (K,) or a['constant'].shape != (K,) or \
            forcing.ndim != 2 or forcing.shape[0] != steps or \
            not (a['norm_src'].shape == a['norm_lo'].shape == a['norm_span'].shape) or \
            not (a['fac_norm'].shape == a['fac_kind'].shape == a['fac_row'].shape == a['fac_degree'].shape) or \
            a['spline_table'].shape[1:] != (499, 4) or bern.ndim != 2 or bern.shape[1] != 21:
        raise ValueError(f"{who}: array shapes disagree")
    struct = _SystemStruct(n_members=E, n_states=K, n_steps=steps, h=float(p['h']), n_forcing_cols=forcing.shape[1],
                           n_norm_forcing=int(p['n_norm_forcing']), n_norm=a['norm_src'].shape[0],
                           n_forcing_factors=int(p['n_forcing_factors']), n_factors=a['fac_norm'].shape[0],
                           n_spline_rows=a['spline_table'].shape[0], n_bern_rows=bern.shape[0], n_entries=a['entries'].shape[0],
                           n_coef=coef.shape[1 if coef_by_draw else 0], **{name: _ptr(arr) for name, arr in a.items()})
    return struct, a


def _control_problem_struct(p, who):
    """The fokl_control_problem of a ``p`` prepared by ``dynamics._prepare_control`` -> (struct, the arrays it points into)."""
    K, P, S, D, nc = int(p['K']), int(p['n_steps']) + 1, int(p['starts']), int(p['D']), int(p['n_controls'])
    a = dict(seg_first=_i32(p['seg_first']), norm_control=_i32(p['norm_control']), ctl_lo=_f64(p['ctl_lo']),
             ctl_width=_f64(p['ctl_width']), ref=_f64(p['ref']), track_weight=_f64(p['wt']), terminal_weight=_f64(p['term']),
             limit_lo=_f64(p['lim_lo']), limit_hi=_f64(p['lim_hi']), move_weight=_f64(p['move']), previous=_f64(p['prev']),
             z0=_f64(p['z0']))
    if a['seg_first'].ndim != 1 or D != nc * a['seg_first'].shape[0] or a['norm_control'].shape != (int(p['n_norm_forcing']),) or \
            any(a[key].shape != (nc,) for key in ('ctl_lo', 'ctl_width', 'move_weight', 'previous')) or a['ref'].shape != (K, P) or \
            any(a[key].shape != (K,) for key in ('track_weight', 'terminal_weight', 'limit_lo', 'limit_hi')) or \
            a['z0'].shape != (S, D):
        raise ValueError(f"{who}: array shapes disagree")
    struct = _ControlProblemStruct(n_controls=nc, n_segments=a['seg_first'].shape[0], limit_weight=float(p['hl']),
                                   has_previous=int(bool(p['has_previous'])), n_starts=S, max_iter=int(p['max_iter']),
                                   tol=float(p['tol']), **{name: _ptr(arr) for name, arr in a.items()})
    return struct, a


def _calibrate_problem_struct(p, who):
    """The fokl_calibrate_problem of a ``p`` prepared by ``dynamics._prepare_calibrate`` -> (struct, the arrays it points into)."""
    E, P, d = int(p['E']), int(p['n_steps']) + 1, int(p['d'])
    a = dict(unknown_src=_i32(p['unknown_src']), norm_param=_i32(p['norm_param']), lo=_f64(p['lo']), hi=_f64(p['hi']),
             prior_mean=_f64(p['prior_mean']), prior_prec=_f64(p['prior_prec']), starts=_f64(p['starts']),
             obs_state=_i32(p['obs_state']), obs_hp=_f64(p['obs_hp']), obs_row=_i32(p['obs_row']), data=_f64(p['data']),
             draw_ids=np.ascontiguousarray(p['draw_ids'], dtype=np.uint32))
    if a['unknown_src'].shape != (d,) or a['norm_param'].shape != (int(p['n_norm_forcing']),) or \
            any(a[key].shape != (d,) for key in ('lo', 'hi', 'prior_mean', 'prior_prec')) or \
            a['starts'].shape != (CALIBRATE_WALKERS, d) or a['obs_state'].ndim != 1 or a['obs_hp'].shape != a['obs_state'].shape or \
            a['data'].ndim != 2 or a['data'].shape[1] != a['obs_state'].shape[0] or a['obs_row'].shape != (P,) or \
            a['draw_ids'].shape != (E,):
        raise ValueError(f"{who}: array shapes disagree")
    struct = _CalibrateProblemStruct(n_unknown=d, n_observed=a['obs_state'].shape[0], n_obs=a['data'].shape[0],
                                     burnin=int(p['burnin']), draws_kept=int(p['draws_kept']), thin=int(p['thin']),
                                     jump_every=int(p['jump_every']), seed=int(p['seed']) & 0xFFFFFFFF,
                                     **{name: _ptr(arr) for name, arr in a.items()})
    return struct, a


class _FirstTrial:
    """The host buffers behind a fokl_control_first_trial, and what they hold as ``dynamics``' ``first_trial`` dict."""

    def __init__(self, S, E, D):
        chunks = -(-E // 64)
        f64 = lambda *shape: np.full(shape, np.nan, dtype=np.float64)
        self.arrays = dict(trial=f64(S, D, 64), slope=f64(S, 64), moved=np.zeros((S, 64), dtype=np.int32), pooled=f64(S, 2 + D),
                           ft=f64(S, E, 64), ft_sums=f64(S, chunks, 64), phi_t=f64(S, 64), a_t=f64(S, 64), z=f64(S, D),
                           status=np.full(S, -1, dtype=np.int32), descent=np.zeros(S, dtype=np.int32))
        self.struct = _FirstTrialStruct(**{name: a.ctypes.data for name, a in self.arrays.items()})

    def ref(self):
        return ctypes.byref(self.struct)

    def result(self, pooled):
        """Lanes 31 and 63 of the wavefront are no trials: [..., 64] -> [..., 2, 31], their ``moved`` apart as
        ``idle_moved`` [S, 2].  ``reached`` [S]: iteration 0 got to its trial pass (it went on, or it stalled there).  ``lane``
        [S]: the wavefront lane whose point became z (0-30 a Newton trial, 32-62 a steepest-descent trial), -1 where none
        passed or the start never got there -- the first moved lane of the half the descent count names whose trial point is
        the new z, bit for bit (an earlier lane at the same point would have the same cost and slope, and would have passed)."""
        a = self.arrays
        halves = lambda x: x.reshape(x.shape[:-1] + (2, 32))[..., :31].copy()
        S, D = a['z'].shape
        status = a['status']
        reached = ~np.isnan(a['pooled'][:, 0])                         # the step kernel writes F only past its stop test
        trial, moved = halves(a['trial']), halves(a['moved']) != 0
        lane = np.full(S, -1, dtype=np.int64)
        for s in np.flatnonzero(reached & (status < 0)):
            half = int(a['descent'][s] > 0)
            same = moved[s, half] & np.all(trial[s, :, half, :] == a['z'][s][:, np.newaxis], axis=0)
            if same.any():
                lane[s] = 32 * half + int(np.argmax(same))
        out = dict(trial=trial, slope=halves(a['slope']), moved=moved, idle_moved=a['moved'][:, [31, 63]].copy(),
                   Ft_draws=halves(a['ft']), F=a['pooled'][:, 0].copy(), noise=a['pooled'][:, 1].copy(), g=a['pooled'][:, 2:].copy(),
                   z=a['z'], status=status, descent_steps=a['descent'], reached=reached, lane=lane)
        if pooled:
            chunk_sums = halves(a['ft_sums'])
            total = chunk_sums[:, 0]
            with np.errstate(all='ignore'):
                for k in range(1, chunk_sums.shape[1]):
                    total = total + chunk_sums[:, k]
            out.update(Ft_chunks=chunk_sums, Ft=total)
        else:
            out.update(phi_t=halves(a['phi_t']), a_t=halves(a['a_t']))
        return out


class DeviceContext:
    """One HIP stream on one MI355X plus the resident dataset and column slots."""

    def __init__(self, device=0):
        self._lib = load()
        h = c_vp(0)
        _check(self._lib.fokl_ctx_create(int(device), ctypes.byref(h)))
        self._h = h
        self.device = device

    def close(self):
        if getattr(self, '_h', None) is not None and self._h:
            self._lib.fokl_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        _check(rc, self._h)

    def sync(self):
        self._ck(self._lib.fokl_sync(self._h))

    # A model whose normalised inputs exist on this context only (upload_staged) is told to fetch them before the dataset
    # is replaced (owner._materialise_inputs()).
    _lazy_owner = None

    def _settle_lazy_inputs(self, keep=None):
        owner, self._lazy_owner = self._lazy_owner, None
        model = owner() if owner is not None else None
        if model is not None and model is not keep:
            model._materialise_inputs()

    def upload(self, x, y, kernel_id, phis_packed, n_basis, width):
        self._settle_lazy_inputs()
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.ascontiguousarray(np.reshape(y, -1), dtype=np.float64)
        if x.ndim != 2 or x.shape[0] != y.shape[0]:
            raise ValueError("inputs must be [n, m] and data [n]")
        phis_packed = np.ascontiguousarray(phis_packed, dtype=np.float64)
        self._ck(self._lib.fokl_upload(self._h, _ptr(x), _ptr(y), x.shape[0], x.shape[1], int(kernel_id),
                                       _ptr(phis_packed), int(n_basis), int(width)))
        self.n, self.m = x.shape

    def stage_inputs(self, x, owner=None):
        """Raw inputs [n, m] (float64, C-contiguous) to the device; -> (column minima, column maxima)."""
        if x.dtype != np.float64 or x.ndim != 2 or not x.flags.c_contiguous:
            raise ValueError("stage_inputs: float64 C-contiguous [n, m] expected")
        self._settle_lazy_inputs(keep=owner)
        lows, highs = np.empty(x.shape[1]), np.empty(x.shape[1])
        self._ck(self._lib.fokl_stage_inputs(self._h, _ptr(x), x.shape[0], x.shape[1], _ptr(lows), _ptr(highs)))
        self._staged_shape = x.shape
        return lows, highs

    def upload_staged(self, y, kernel_id, phis_packed, n_basis, width, lows, spans, owner=None):
        """fokl_upload from the staged raw inputs, normalised on the device as (x - lows) / spans.  owner: the model whose
        ``inputs`` these are (asked to fetch them before the next dataset replaces them here)."""
        n, m = self._staged_shape
        y = np.ascontiguousarray(np.reshape(y, -1), dtype=np.float64)
        if y.shape[0] != n:
            raise ValueError("inputs must be [n, m] and data [n]")
        phis_packed = np.ascontiguousarray(phis_packed, dtype=np.float64)
        lows, spans = np.ascontiguousarray(lows, dtype=np.float64), np.ascontiguousarray(spans, dtype=np.float64)
        self._ck(self._lib.fokl_upload_staged(self._h, _ptr(y), n, m, int(kernel_id), _ptr(phis_packed), int(n_basis),
                                              int(width), _ptr(lows), _ptr(spans)))
        self.n, self.m = n, m
        if owner is not None:
            import weakref
            self._lazy_owner = weakref.ref(owner)

    def download_inputs(self):
        out = np.empty((getattr(self, 'n', 0) or 1, getattr(self, 'm', 0) or 1), dtype=np.float64)   # (no dataset: the call says so)
        self._ck(self._lib.fokl_download_inputs(self._h, _ptr(out)))
        return out

    def reserve_slots(self, n_slots):
        self._ck(self._lib.fokl_reserve_slots(self._h, int(n_slots)))

    @property
    def slot_capacity(self):
        return self._lib.fokl_slot_capacity(self._h)

    def build_terms(self, terms, slots):
        terms = np.ascontiguousarray(np.atleast_2d(terms), dtype=np.int32)
        slots = np.ascontiguousarray(slots, dtype=np.int32)
        if terms.shape[0] != slots.shape[0]:
            raise ValueError("one slot per term")
        self._ck(self._lib.fokl_build_terms(self._h, _ptr(terms), terms.shape[0], _ptr(slots)))

    def build_terms_deriv(self, terms, slots, wrt_input, order, divisor):
        terms = np.ascontiguousarray(np.atleast_2d(terms), dtype=np.int32)
        slots = np.ascontiguousarray(slots, dtype=np.int32)
        if terms.shape[0] != slots.shape[0]:
            raise ValueError("one slot per term")
        self._ck(self._lib.fokl_build_terms_deriv(self._h, _ptr(terms), terms.shape[0], _ptr(slots), int(wrt_input),
                                                  int(order), float(divisor)))

    def gram(self, row_slots, col_slots, path=0, allreduce=False):
        rs = np.ascontiguousarray(row_slots, dtype=np.int32)
        cs = np.ascontiguousarray(col_slots, dtype=np.int32)
        out = np.empty((rs.shape[0], cs.shape[0]), dtype=np.float64)
        self._ck(self._lib.fokl_gram(self._h, _ptr(rs), rs.shape[0], _ptr(cs), cs.shape[0], _ptr(out), int(path),
                                     int(bool(allreduce))))
        return out

    def gram_launch(self, row_slots, col_slots, allreduce=False):
        """fokl_gram_launch: -> shape of the block gram_fetch will return."""
        rs = np.ascontiguousarray(row_slots, dtype=np.int32)
        cs = np.ascontiguousarray(col_slots, dtype=np.int32)
        self._ck(self._lib.fokl_gram_launch(self._h, _ptr(rs), rs.shape[0], _ptr(cs), cs.shape[0],
                                            int(bool(allreduce))))
        return rs.shape[0], cs.shape[0]

    def gram_ready(self):
        """True once gram_fetch would not wait."""
        rc = self._lib.fokl_gram_ready(self._h)
        if rc < 0:
            self._ck(rc)
        return rc == 1

    def gram_fetch(self, shape):
        out = np.empty(shape, dtype=np.float64)
        self._ck(self._lib.fokl_gram_fetch(self._h, _ptr(out), out.size))
        return out

    def bic_resid(self, slots, betahat, allreduce=False):
        s = np.ascontiguousarray(slots, dtype=np.int32)
        bh = np.ascontiguousarray(np.reshape(betahat, -1), dtype=np.float64)
        if s.shape[0] != bh.shape[0]:
            raise ValueError("one coefficient per column")
        out = np.empty(2, dtype=np.float64)
        self._ck(self._lib.fokl_bic_resid(self._h, _ptr(s), s.shape[0], _ptr(bh), _ptr(out), int(bool(allreduce))))
        return out[0], out[1]

    def bic_resid_launch(self, slots, betahat):
        s = np.ascontiguousarray(slots, dtype=np.int32)
        bh = np.ascontiguousarray(np.reshape(betahat, -1), dtype=np.float64)
        if s.shape[0] != bh.shape[0]:
            raise ValueError("one coefficient per column")
        self._ck(self._lib.fokl_bic_resid_launch(self._h, _ptr(s), s.shape[0], _ptr(bh)))

    def bic_resid_terms_launch(self, terms, betahat):
        """Matrix-free residual pass of the model [intercept] + terms (rows of the interaction matrix)."""
        terms = np.ascontiguousarray(terms, dtype=np.int32)
        beta = np.ascontiguousarray(np.reshape(betahat, -1), dtype=np.float64)
        n_terms = terms.shape[0] if terms.size else 0
        if beta.shape[0] != n_terms + 1:
            raise ValueError("betahat needs one coefficient for the intercept and one per term")
        self._ck(self._lib.fokl_bic_resid_terms_launch(self._h, _ptr(terms), n_terms, _ptr(beta)))

    def bic_resid_fetch(self, allreduce=False):
        out = np.empty(2, dtype=np.float64)
        self._ck(self._lib.fokl_bic_resid_fetch(self._h, _ptr(out), int(bool(allreduce))))
        return out[0], out[1]

    def predict(self, slots, betas, cut=None):
        s = np.ascontiguousarray(slots, dtype=np.int32)
        betas = np.ascontiguousarray(betas, dtype=np.float64)
        draws, nc = betas.shape
        if nc != s.shape[0]:
            raise ValueError("betas columns must match the slot list")
        mean = np.empty(self.n, dtype=np.float64)
        bounds = np.empty((self.n, 2), dtype=np.float64) if cut is not None else None
        self._ck(self._lib.fokl_predict(self._h, _ptr(s), nc, _ptr(betas), draws, int(cut or 0), _ptr(mean),
                                        _ptr(bounds)))
        return (mean, bounds) if cut is not None else mean

    def predict_report(self):
        """What the last ``predict`` on this context ran (fokl_predict_report): ``kernel`` (PREDICT_*), ``wide`` (basis values
        read from the columns, not from LDS), ``grid`` workgroups over ``tiles`` row tiles (16 rows on the matrix-pipe
        kernel, 64 on the VALU kernel), and of the matrix-pipe kernel's ``tiles_done`` the ``tiles_fallback`` that went
        through its exact fallback pass (both 0 for the VALU kernel).  PREDICT_NONE and zeros after a refused call."""
        out = np.zeros(6, dtype=np.int64)
        self._ck(self._lib.fokl_predict_report(self._h, _ptr(out)))
        return dict(kernel=int(out[0]), wide=bool(out[1]), grid=int(out[2]), tiles=int(out[3]), tiles_done=int(out[4]),
                    tiles_fallback=int(out[5]))

    def population_stats(self, slots, betas, shift, cuts=None, with_data=False):
        """fokl_population_stats over the uploaded rows: the columns ``slots`` times every row of ``betas`` [E, nc], reduced
        over the ROWS per draw -> (moments [E, 6] = sum(y - c), sum((y - c)^2), min, max, sum(e), sum(e^2) with c = ``shift``
        [E] and e = the uploaded y - y (zeros without ``with_data``), above [E, K] int64 = rows with y > ``cuts`` [E, K],
        K <= 32).  Two calls with the same arguments return the same bits."""
        s = np.ascontiguousarray(slots, dtype=np.int32)
        betas = np.ascontiguousarray(betas, dtype=np.float64)
        if betas.ndim != 2 or betas.shape[1] != s.shape[0]:
            raise ValueError("betas columns must match the slot list")
        E = betas.shape[0]
        shift = np.ascontiguousarray(shift, dtype=np.float64)
        cuts = np.zeros((E, 0)) if cuts is None else np.ascontiguousarray(cuts, dtype=np.float64)
        if shift.shape != (E,) or cuts.ndim != 2 or cuts.shape[0] != E or cuts.shape[1] > POPULATION_MAX_CUTS:
            raise ValueError("population_stats: one shift and at most 32 cut points per draw")
        K = cuts.shape[1]
        moments = np.empty((E, 6), dtype=np.float64)
        above = np.zeros((E, K), dtype=np.int64)
        self._ck(self._lib.fokl_population_stats(self._h, _ptr(s), s.shape[0], _ptr(betas), E, _ptr(shift),
                                                 _ptr(cuts) if K else None, K, int(bool(with_data)), _ptr(moments),
                                                 _ptr(above) if K else None))
        return moments, above

    def population_report(self):
        """What the last ``population_stats`` on this context ran (fokl_population_report): ``coefficients`` ('registers':
        a wavefront kept its draws' coefficients for the whole launch; 'table': read one k-step ahead, models wider than 128
        columns), the ``grid`` of workgroups = ``chunks`` (rounded up to 8) x ``draw_blocks`` of 128 draws,
        ``tiles_per_chunk`` of the ``row_tiles`` 16-row tiles, ``lds_bytes`` and the ``pieces`` the columns were walked in.
        'none' and zeros after a refused call."""
        out = np.zeros(8, dtype=np.int64)
        self._ck(self._lib.fokl_population_report(self._h, _ptr(out)))
        v = [int(x) for x in out]
        return dict(coefficients=POPULATION_COEFFICIENTS[v[0]], grid=v[1], draw_blocks=v[2], chunks=v[3],
                    tiles_per_chunk=v[4], row_tiles=v[5], lds_bytes=v[6], pieces=v[7])

    def resample_chains(self, lamb, qty, shift, astar, atau_star, b, btau, dtd, sigsqd0, tausqd0, burnin, draws, thin, seed,
                        rows=True, chains_per_group=0, attempt_cap=0):
        """fokl_resample_chains: one Gibbs chain per entry of ``sigsqd0`` / ``tausqd0`` in the eigenbasis (lamb, qty [P + 1]),
        burnin + draws iterations each -> dict(w [chains, kept, P + 1], sigsqd, tausqd, attempts [chains, kept] -- None
        without ``rows`` --, sums [chains, 3, 2, P + 3], counts [chains, 4]); resample.resample_host is its statement and
        documents the fields.  ``chains_per_group`` / ``attempt_cap``: 0 the defaults; test hooks."""
        lamb, qty, shift, sigsqd0, tausqd0 = (np.ascontiguousarray(np.reshape(v, -1), dtype=np.float64)
                                              for v in (lamb, qty, shift, sigsqd0, tausqd0))
        p1, chains = lamb.shape[0], sigsqd0.shape[0]
        if qty.shape[0] != p1 or shift.shape[0] != p1 or tausqd0.shape[0] != chains:
            raise ValueError("resample_chains: lamb, qty, shift [P + 1] and one start per chain")
        burnin, draws, thin = int(burnin), int(draws), int(thin)
        if draws < 1 or thin < 1:
            raise ValueError("resample_chains: draws >= 1 and thin >= 1")
        kept = -(-draws // thin)
        w = sig = tau = att = None
        if rows:
            w = np.empty((chains, kept, p1), dtype=np.float64)
            sig, tau = np.empty((chains, kept), dtype=np.float64), np.empty((chains, kept), dtype=np.float64)
            att = np.empty((chains, kept), dtype=np.int32)
        sums = np.empty((chains, RESAMPLE_SEGMENTS, 2, p1 + 2), dtype=np.float64)
        counts = np.empty((chains, 4), dtype=np.int64)
        self._ck(self._lib.fokl_resample_chains(self._h, p1, _ptr(lamb), _ptr(qty), _ptr(shift), float(astar), float(atau_star),
                                                float(b), float(btau), float(dtd), chains, _ptr(sigsqd0), _ptr(tausqd0), burnin,
                                                draws, thin, int(seed) & 0xFFFFFFFF, int(chains_per_group), int(attempt_cap),
                                                _ptr(w), _ptr(sig), _ptr(tau), _ptr(att), _ptr(sums), _ptr(counts)))
        return dict(w=w, sigsqd=sig, tausqd=tau, attempts=att, sums=sums, counts=counts)

    def resample_report(self):
        """What the last ``resample_chains`` on this context ran (fokl_resample_report): ``instance`` (the kernel's
        eigen-coordinates per lane: 1, 2, 3, 4, 6, 8 or 12), ``chains``, ``iterations`` per chain (burn-in included),
        ``chains_per_group`` (wavefronts per workgroup), the ``grid``, Marsaglia-Tsang ``attempts`` in all and
        ``attempts_max`` (the most one gamma variate needed), ``kernel_ms``, ``flagged`` chains and the rows ``kept`` per
        chain.  Zeros after a refused call."""
        out = np.zeros(10, dtype=np.int64)
        self._ck(self._lib.fokl_resample_report(self._h, _ptr(out)))
        v = [int(x) for x in out]
        return dict(instance=v[0], chains=v[1], iterations=v[2], chains_per_group=v[3], attempts=v[4], attempts_max=v[5],
                    kernel_ms=v[6] / 1000.0, grid=v[7], flagged=v[8], kept=v[9])

    def robust_pass(self, slots, weights, beta, sigsqd, nu, seed, chain, iteration, attempt_cap=0, want_rows=True):
        """fokl_robust_pass over the uploaded rows: one row pass of chain ``chain`` at ``iteration`` over the columns ``slots``
        (the intercept's included) and the uploaded y, ``weights`` [n] or None -> (G [nc + 1, nc + 1], lam [n], attempts [n]
        int32; the last two None without ``want_rows``).  robust.pass_host is its statement."""
        s = np.ascontiguousarray(slots, dtype=np.int32)
        nc = s.shape[0]
        w = None if weights is None else np.ascontiguousarray(np.reshape(weights, -1), dtype=np.float64)
        b = None if beta is None else np.ascontiguousarray(np.reshape(beta, -1), dtype=np.float64)
        if b is not None and b.shape[0] != nc:
            raise ValueError("robust_pass: one coefficient per slot")
        G = np.empty((nc + 1, nc + 1), dtype=np.float64)
        lam = np.empty(self.n, dtype=np.float64) if want_rows else None
        att = np.empty(self.n, dtype=np.int32) if want_rows else None
        self._ck(self._lib.fokl_robust_pass(self._h, _ptr(s), nc, _ptr(w), 0 if w is None else w.shape[0], _ptr(b), float(sigsqd),
                                            float(nu), int(seed) & 0xFFFFFFFF, int(chain), int(iteration), int(attempt_cap),
                                            _ptr(G), _ptr(lam), _ptr(att)))
        return G, lam, att

    def robust_step(self, G, sigsqd, tausqd, hyper, seed, chain, iteration, attempt_cap=0):
        """fokl_robust_step on a given G [nc + 1, nc + 1] (its upper triangle is read) -> (beta [nc], sigsqd, tausqd, flag);
        ``hyper``: dict(astar, atau_star, b, btau).  robust.step_host is its statement."""
        G = np.ascontiguousarray(G, dtype=np.float64)
        if G.ndim != 2 or G.shape[0] != G.shape[1] or G.shape[0] < 2:
            raise ValueError("robust_step: G must be [nc + 1, nc + 1]")
        nc = G.shape[0] - 1
        beta, state, counts = np.empty(nc, dtype=np.float64), np.empty(2, dtype=np.float64), np.empty(4, dtype=np.int64)
        self._ck(self._lib.fokl_robust_step(self._h, nc, _ptr(G), float(sigsqd), float(tausqd), float(hyper['astar']),
                                            float(hyper['atau_star']), float(hyper['b']), float(hyper['btau']),
                                            int(seed) & 0xFFFFFFFF, int(chain), int(iteration), int(attempt_cap), _ptr(beta),
                                            _ptr(state), _ptr(counts)))
        return beta, float(state[0]), float(state[1]), int(counts[1])

    def robust_chains(self, slots, weights, nu, hyper, shift, sigsqd0, tausqd0, burnin, draws, thin, seed, rows=True,
                      attempt_cap=0, chain_ids=None, want_lam=True):
        """fokl_robust_chains over the uploaded rows: one chain per entry of ``sigsqd0`` / ``tausqd0``, burnin + draws iterations
        of pass, reduce and step each -> dict(betas [chains, kept, nc], sigsqd, tausqd [chains, kept], attempts [chains, kept]
        int64 -- None without ``rows`` --, sums [chains, 3, 2, nc + 2], counts [chains, 4], lam_sum [chains, n]);
        robust.robust_host is its statement and documents the fields."""
        s = np.ascontiguousarray(slots, dtype=np.int32)
        nc = s.shape[0]
        w = None if weights is None else np.ascontiguousarray(np.reshape(weights, -1), dtype=np.float64)
        shift, sigsqd0, tausqd0 = (np.ascontiguousarray(np.reshape(v, -1), dtype=np.float64) for v in (shift, sigsqd0, tausqd0))
        chains = sigsqd0.shape[0]
        if shift.shape[0] != nc or tausqd0.shape[0] != chains:
            raise ValueError("robust_chains: shift [nc] and one start per chain")
        ids = None if chain_ids is None else np.ascontiguousarray(np.reshape(chain_ids, -1), dtype=np.int32)
        if ids is not None and ids.shape[0] != chains:
            raise ValueError("robust_chains: one chain id per chain")
        burnin, draws, thin = int(burnin), int(draws), int(thin)
        if draws < 1 or thin < 1:
            raise ValueError("robust_chains: draws >= 1 and thin >= 1")
        kept = -(-draws // thin)
        betas = sig = tau = att = None
        if rows:
            betas = np.empty((chains, kept, nc), dtype=np.float64)
            sig, tau = np.empty((chains, kept), dtype=np.float64), np.empty((chains, kept), dtype=np.float64)
            att = np.empty((chains, kept), dtype=np.int64)
        sums = np.empty((chains, RESAMPLE_SEGMENTS, 2, nc + 2), dtype=np.float64)
        counts = np.empty((chains, 4), dtype=np.int64)
        lam_sum = np.empty((chains, self.n), dtype=np.float64) if want_lam else None
        self._ck(self._lib.fokl_robust_chains(self._h, _ptr(s), nc, _ptr(w), 0 if w is None else w.shape[0], float(nu),
                                              float(hyper['astar']), float(hyper['atau_star']), float(hyper['b']),
                                              float(hyper['btau']), _ptr(shift), chains, _ptr(ids), _ptr(sigsqd0), _ptr(tausqd0),
                                              burnin, draws, thin, int(seed) & 0xFFFFFFFF, int(attempt_cap), _ptr(betas), _ptr(sig),
                                              _ptr(tau), _ptr(att), _ptr(sums), _ptr(counts), _ptr(lam_sum)))
        return dict(betas=betas, sigsqd=sig, tausqd=tau, attempts=att, sums=sums, counts=counts, lam_sum=lam_sum)

    def robust_report(self):
        """What the last ``robust_pass`` / ``robust_step`` / ``robust_chains`` on this context ran (fokl_robust_report): the
        ``grid`` (workgroups of the pass per chain, chains), the ``partials`` per chain and the doubles of one, ``lds_bytes``
        of the pass and of the step, ``columns`` of [X|y] and their 16-column ``blocks``, ``iterations``, rows ``kept`` per
        chain, Marsaglia-Tsang ``attempts``, ``flagged`` chains, and the kernel time: ``pass_ms``, ``reduce_ms``, ``step_ms``
        summed over the ``timed_iterations`` last iterations, ``total_ms`` of the whole run.  Zeros after a refused call."""
        out = np.zeros(16, dtype=np.int64)
        self._ck(self._lib.fokl_robust_report(self._h, _ptr(out)))
        v = [int(x) for x in out]
        return dict(grid=(v[0], v[1]), partials=v[0], partial_doubles=v[2], lds_bytes=v[3], step_lds_bytes=v[4], columns=v[5],
                    blocks=v[6], iterations=v[7], kept=v[8], attempts=v[9], flagged=v[10], pass_ms=v[11] / 1000.0,
                    reduce_ms=v[12] / 1000.0, step_ms=v[13] / 1000.0, timed_iterations=v[14], total_ms=v[15] / 1000.0)

    def _sw(self, sw, who):
        """``sw`` [rows] (sqrt of the rows' precisions) as the noise entry points take it, or None."""
        if sw is None:
            return None
        sw = np.ascontiguousarray(np.reshape(sw, -1), dtype=np.float64)
        if sw.shape[0] != self.n:
            raise ValueError(f"{who}: sw holds {sw.shape[0]} values, {self.n} rows are uploaded")
        return sw

    def score_rows_noise(self, slots, betas, sigsqd, want_loo=True, want_tail=False, nu=np.inf, sw=None):
        """fokl_score_rows_noise: ``score_rows`` under Student-t noise with ``nu`` degrees of freedom (np.inf: Gaussian) and
        row precisions ``sw`` [rows] = sqrt(w) (None: ones).  score.score_rows_host(nu=, sw=) is its statement.  nu = inf with
        sw = None is routed to ``score_rows``' instances and returns its bits."""
        return self.score_rows(slots, betas, sigsqd, want_loo, want_tail, _noise=(float(nu), self._sw(sw, 'score_rows_noise')))

    def score_rows(self, slots, betas, sigsqd, want_loo=True, want_tail=False, _noise=None):
        """fokl_score_rows over the uploaded rows: ll[i, d] of the uploaded y against the columns ``slots`` times every row of
        ``betas`` [E, nc] with ``sigsqd`` [E], reduced over the DRAWS per row -> stats [S, 8] = lppd, ll_mean, p_waic and, with
        ``want_loo`` (else zeros), elpd_loo, khat, sigma, max r, M'; with ``want_tail`` also the sorted top M + 1 shifted
        log ratios [S, M + 1].  score.score_rows_host is its statement.  Two calls with the same arguments return the same
        bits."""
        s = np.ascontiguousarray(slots, dtype=np.int32)
        betas = np.ascontiguousarray(betas, dtype=np.float64)
        if betas.ndim != 2 or betas.shape[1] != s.shape[0]:
            raise ValueError("betas columns must match the slot list")
        E = betas.shape[0]
        sigsqd = np.ascontiguousarray(np.reshape(sigsqd, -1), dtype=np.float64)
        if sigsqd.shape[0] != E:
            raise ValueError("score_rows: one sigsqd per row of betas")
        stats = np.empty((self.n, 8), dtype=np.float64)
        tail = None
        if want_tail:
            M = int(min(E // 5, np.ceil(3.0 * np.sqrt(E))))
            tail = np.empty((self.n, M + 1), dtype=np.float64)
        if _noise is not None:
            self._ck(self._lib.fokl_score_rows_noise(self._h, _ptr(s), s.shape[0], _ptr(betas), _ptr(sigsqd), E,
                                                     int(bool(want_loo)), _ptr(stats), _ptr(tail), _noise[0], _ptr(_noise[1])))
        else:
            self._ck(self._lib.fokl_score_rows(self._h, _ptr(s), s.shape[0], _ptr(betas), _ptr(sigsqd), E, int(bool(want_loo)),
                                               _ptr(stats), _ptr(tail)))
        return (stats, tail) if want_tail else stats

    def score_report(self):
        """What the last ``score_rows`` on this context ran (fokl_score_report): ``instance`` ('waic': no list, 'waic_loo'),
        the ``grid`` of one-wavefront workgroups over ``row_tiles`` 16-row tiles, ``lds_bytes``, the ``tail_capacity`` used
        (M + 1; 0 without want_loo), the ``raw_rows`` that took the khat = inf branch, ``kernel_ms`` and the ``noise``
        instance ('gaussian', 'gaussian_weighted', 'student').  'none' and zeros after a refused call."""
        out = np.zeros(8, dtype=np.int64)
        self._ck(self._lib.fokl_score_report(self._h, _ptr(out)))
        v = [int(x) for x in out]
        return dict(instance=SCORE_INSTANCES[v[0]], grid=v[1], row_tiles=v[2], lds_bytes=v[3], tail_capacity=v[4],
                    raw_rows=v[5], kernel_ms=v[6] / 1000.0, noise=NOISES[v[7]])

    def predictive_rows_noise(self, slots, betas, sd, rinv, with_data, p, z, max_passes=32, ftol=1e-13, xtol=1e-15, nu=np.inf,
                              sw=None):
        """fokl_predictive_rows_noise: ``predictive_rows`` for mixtures of t_nu components (``nu`` finite, at most
        PREDICTIVE_NU_MAX; ``z`` are then quantiles of the standard t_nu) with the scale sd_d / sw_i, ``sw`` [rows] = sqrt of
        the rows' precisions (None: ones).  predictive.predictive_rows_host(nu=, sw=) is its statement.  nu = inf with sw =
        None is routed to ``predictive_rows``' instances and returns its bits."""
        return self.predictive_rows(slots, betas, sd, rinv, with_data, p, z, max_passes, ftol, xtol,
                                    _noise=(float(nu), self._sw(sw, 'predictive_rows_noise')))

    def predictive_rows(self, slots, betas, sd, rinv, with_data, p, z, max_passes=32, ftol=1e-13, xtol=1e-15, _noise=None):
        """fokl_predictive_rows over the uploaded rows: the mixture over the rows of ``betas`` [E, nc] of N(X_i . beta_d,
        sd_d^2) per uploaded row, ``sd`` [E] and ``rinv`` [E] = 1 / (sd sqrt(2)) as the caller formed them, the uploaded y read
        only ``with_data``; ``p`` [Q] and their standard normal quantiles ``z`` [Q], Q <= 8 -> the block [S, 6 + 5 Q] = mu_0,
        s1, s2, min mu, max mu, pit, then per quantile q, residual, lo, hi, passes.  predictive.predictive_rows_host is its
        statement.  Two calls with the same arguments return the same bits."""
        s = np.ascontiguousarray(slots, dtype=np.int32)
        betas = np.ascontiguousarray(betas, dtype=np.float64)
        if betas.ndim != 2 or betas.shape[1] != s.shape[0]:
            raise ValueError("betas columns must match the slot list")
        E = betas.shape[0]
        sd = np.ascontiguousarray(np.reshape(sd, -1), dtype=np.float64)
        rinv = np.ascontiguousarray(np.reshape(rinv, -1), dtype=np.float64)
        if sd.shape[0] != E or rinv.shape[0] != E:
            raise ValueError("predictive_rows: one sd and one rinv per row of betas")
        p = np.ascontiguousarray(np.reshape(p, -1), dtype=np.float64)
        z = np.ascontiguousarray(np.reshape(z, -1), dtype=np.float64)
        if z.shape[0] != p.shape[0]:
            raise ValueError("predictive_rows: one z per p")
        Q = p.shape[0]
        out = np.empty((self.n, 6 + 5 * Q), dtype=np.float64)
        args = (self._h, _ptr(s), s.shape[0], _ptr(betas), _ptr(sd), _ptr(rinv), E, float(np.mean(sd * sd)), int(bool(with_data)),
                _ptr(p) if Q else None, _ptr(z) if Q else None, Q, int(max_passes), float(ftol), float(xtol), _ptr(out))
        if _noise is not None:
            self._ck(self._lib.fokl_predictive_rows_noise(*args, _noise[0], _ptr(_noise[1])))
        else:
            self._ck(self._lib.fokl_predictive_rows(*args))
        return out

    def predictive_report(self):
        """What the last ``predictive_rows`` on this context ran (fokl_predictive_report): ``instance`` ('pit': data only,
        'quantiles', 'pit_quantiles'), ``with_data`` and ``with_quantiles``, the ``grid`` of one-wavefront workgroups over
        ``row_tiles`` 16-row tiles, ``lds_bytes``, ``quantiles`` (Q), ``passes_max`` (the most passes any tile ran; pass 0 is
        not counted), ``passes_sum`` (over the tiles), the ``unresolved`` pairs, ``kernel_ms`` and the ``noise`` instance
        ('gaussian', 'gaussian_weighted', 'student').  'none' and zeros after a refused call."""
        out = np.zeros(10, dtype=np.int64)
        self._ck(self._lib.fokl_predictive_report(self._h, _ptr(out)))
        v = [int(x) for x in out]
        return dict(instance=PREDICTIVE_INSTANCES[v[0]], with_data=bool(v[0] & 1), with_quantiles=bool(v[0] & 2), grid=v[1],
                    row_tiles=v[2], lds_bytes=v[3], quantiles=v[4], passes_max=v[5], passes_sum=v[6], unresolved=v[7],
                    kernel_ms=v[8] / 1000.0, noise=NOISES[v[9]])

    def design_select(self, slots, C0, CMC0=None, picks=1, replicates=False, refresh_every=64, keep=False, grid_cap=0):
        """fokl_design_select over the uploaded rows (the pool): greedy selection of ``picks`` rows given C0 = (G + I / tau^2)^-1
        [nc, nc] and, for integrated variance reduction, CMC0 = C0 M C0 (None: greedy D-optimal) -> dict(index [picks] int64,
        gain [picks], vstar [picks], x [picks, nc] and, with ``keep``, v [S] (and w [S] with CMC0) after the last pick).
        design.select_host is its statement: on integer data the first pick (index, gain, vstar, x), the first downdate (v
        and w with ``picks=1, keep=True``) and the second pick's index and gain are its bits, everything later is equal to
        rounding (C is no longer integer after a pick).  A pick that finds no row (all masked, or every criterion NaN) is
        index -1, gain -inf, x = 0.  ``grid_cap``: 0 the device's grids; a test hook.  Two calls with the same arguments
        return the same bits."""
        s = np.ascontiguousarray(slots, dtype=np.int32)
        nc = s.shape[0]
        C0 = np.ascontiguousarray(C0, dtype=np.float64)
        if C0.shape != (nc, nc):
            raise ValueError("design_select: C0 must be [columns, columns] of the slot list")
        if CMC0 is not None:
            CMC0 = np.ascontiguousarray(CMC0, dtype=np.float64)
            if CMC0.shape != (nc, nc):
                raise ValueError("design_select: CMC0 must be [columns, columns] of the slot list")
        picks = int(picks)
        rows = max(picks, 0)
        index = np.empty(rows, dtype=np.int64)
        gain, vstar, x = np.empty(rows), np.empty(rows), np.empty((rows, nc))
        v = np.empty(self.n, dtype=np.float64) if keep else None
        w = np.empty(self.n, dtype=np.float64) if keep and CMC0 is not None else None
        self._ck(self._lib.fokl_design_select(self._h, _ptr(s), nc, _ptr(C0), _ptr(CMC0), picks, int(bool(replicates)),
                                              int(refresh_every), int(grid_cap), _ptr(index), _ptr(gain), _ptr(vstar), _ptr(x),
                                              _ptr(v), _ptr(w)))
        return dict(index=index, gain=gain, vstar=vstar, x=x, v=v, w=w)

    def design_report(self):
        """What the last ``design_select`` on this context ran (fokl_design_report): ``instance`` ('variance', 'ivr'), the
        ``grid`` of one-wavefront workgroups of the quadratic-form kernel over ``row_tiles`` 16-row tiles and its
        ``lds_bytes``, the ``step_grid``, the ``picks``, the ``refreshes`` (quadratic-form launches after the first), the
        ``launches`` in all, ``kernel_us`` of the whole queue and ``quadform_us`` of the quadratic-form launches; ``step_us``
        and ``pivot_us`` are measured while the context's timing is enabled (else 0).  'none' and zeros after a refused
        call."""
        out = np.zeros(12, dtype=np.int64)
        self._ck(self._lib.fokl_design_report(self._h, _ptr(out)))
        v = [int(x) for x in out]
        return dict(instance=DESIGN_INSTANCES[v[0]], grid=v[1], step_grid=v[2], row_tiles=v[3], lds_bytes=v[4], picks=v[5],
                    refreshes=v[6], launches=v[7], kernel_us=v[8], quadform_us=v[9], step_us=v[10], pivot_us=v[11])

    def acquire_select(self, slots, betas, incumbent, picks=1, criterion='ei', lazy=True, grid_cap=0, trace_pick=-1):
        """fokl_acquire_select over the uploaded rows (the pool): greedy selection of ``picks`` rows by expected improvement
        ('ei') or probability of improvement ('pi') over the rows of ``betas`` [E, nc] given the incumbent [E] of every draw
        (finite or -inf), sense 'max' -> dict(index [picks] int64, gain [picks], incumbent_after [E], tiles_evaluated [picks]
        int64 and, with ``trace_pick=k``, trace_g [S] -- every row's gain as it stood when pick k was taken -- and, under
        ``lazy``, trace_eval [tiles] uint8; else None).  acquire.select_host is its statement: on integer data every field is
        its bits.  A pick that finds no row (every gain NaN) is index -1, gain -inf.  ``report['launches']`` is 2 per pick
        without ``lazy``, 2 + 4 (picks - 1) with it; nothing waits on the host between them.  ``grid_cap``: 0 the device's
        grids; a test hook.  Two calls with the same arguments return the same bits."""
        s = np.ascontiguousarray(slots, dtype=np.int32)
        nc = s.shape[0]
        betas = np.ascontiguousarray(betas, dtype=np.float64)
        if betas.ndim != 2 or betas.shape[1] != nc:
            raise ValueError("betas columns must match the slot list")
        E = betas.shape[0]
        incumbent = np.ascontiguousarray(np.reshape(incumbent, -1), dtype=np.float64)
        if incumbent.shape[0] != E:
            raise ValueError("acquire_select: one incumbent per row of betas")
        if criterion not in ACQUIRE_INSTANCES[1:]:
            raise ValueError(f"acquire_select: criterion must be one of {ACQUIRE_INSTANCES[1:]}")
        picks, trace_pick = int(picks), int(trace_pick)
        rows = max(picks, 0)
        index, tiles = np.empty(rows, dtype=np.int64), np.empty(rows, dtype=np.int64)
        gain, after = np.empty(rows), np.empty(E)
        trace_g = np.empty(self.n, dtype=np.float64) if trace_pick >= 0 else None
        trace_eval = np.empty(-(-self.n // 16), dtype=np.uint8) if trace_pick >= 0 and lazy else None
        self._ck(self._lib.fokl_acquire_select(self._h, _ptr(s), nc, _ptr(betas), E, _ptr(incumbent),
                                               ACQUIRE_INSTANCES.index(criterion), int(bool(lazy)), picks, int(grid_cap),
                                               trace_pick, _ptr(index), _ptr(gain), _ptr(after), _ptr(tiles), _ptr(trace_g),
                                               _ptr(trace_eval)))
        return dict(index=index, gain=gain, incumbent_after=after, tiles_evaluated=tiles, trace_g=trace_g, trace_eval=trace_eval)

    def acquire_report(self):
        """What the last ``acquire_select`` on this context ran (fokl_acquire_report): ``instance`` ('ei', 'pi'), ``lazy``,
        the ``grid`` of one-wavefront workgroups of the pass kernel over ``row_tiles`` 16-row tiles and its ``lds_bytes``, the
        ``bound_grid``, ``dt`` (16-draw tiles per block of the product), the ``picks``, the ``launches`` in all,
        ``tiles_evaluated`` over all picks, ``tiles_evaluated_max_lazy`` (by the most expensive pick after the first under
        ``lazy``), ``kernel_us`` of the whole queue; ``pass_us``, ``bound_us`` and ``pivot_us`` are measured while the
        context's timing is enabled (else 0).  'none' and zeros after a refused call."""
        out = np.zeros(15, dtype=np.int64)
        self._ck(self._lib.fokl_acquire_report(self._h, _ptr(out)))
        v = [int(x) for x in out]
        return dict(instance=ACQUIRE_INSTANCES[v[0]], lazy=bool(v[1]), grid=v[2], bound_grid=v[3], row_tiles=v[4], lds_bytes=v[5],
                    dt=v[6], picks=v[7], launches=v[8], tiles_evaluated=v[9], tiles_evaluated_max_lazy=v[10], kernel_us=v[11],
                    pass_us=v[12], bound_us=v[13], pivot_us=v[14])

    def _acquire_system_arguments(self, who, slots, betas, lo, hi):
        """The models of ``acquire_system_select`` / ``acquire_system_incumbent`` as the library takes them: slots and betas
        one model behind the other, the widths, the limits."""
        slots = [np.ascontiguousarray(s, dtype=np.int32).reshape(-1) for s in slots]
        betas = [np.ascontiguousarray(b, dtype=np.float64) for b in betas]
        if len(slots) != len(betas) or len(slots) < 1:
            raise ValueError(f"{who}: one slot list and one betas per model")
        E = betas[0].shape[0] if betas[0].ndim == 2 else -1
        for s, b in zip(slots, betas):
            if b.ndim != 2 or b.shape[1] != s.shape[0] or b.shape[0] != E:
                raise ValueError(f"{who}: every model's betas must be [E, its slots], with one E")
        lo = np.ascontiguousarray(np.reshape(lo, -1), dtype=np.float64)
        hi = np.ascontiguousarray(np.reshape(hi, -1), dtype=np.float64)
        if lo.shape[0] != len(slots) - 1 or hi.shape[0] != len(slots) - 1:
            raise ValueError(f"{who}: one (lo, hi) per constraint model, i.e. per model after the first")
        widths = np.array([s.shape[0] for s in slots], dtype=np.int32)
        return (np.ascontiguousarray(np.concatenate(slots)), widths, np.ascontiguousarray(np.concatenate([b.ravel() for b in betas])),
                E, lo, hi)

    def acquire_system_select(self, slots, betas, incumbent, lo, hi, picks=1, criterion='ei', lazy=True, grid_cap=0,
                              trace_pick=-1):
        """fokl_acquire_system_select over the uploaded rows (the pool): ``acquire_select`` under limits on other models'
        outputs.  ``slots`` = [objective's slots, constraint model 1's, ...], ``betas`` = [B0 [E, nc_0], B1 [E, nc_1], ...],
        ``lo`` / ``hi`` [K] the limits of the constraint models (infinite: none) -> ``acquire_select``'s dict and feasible
        [picks] int64, the draws in which each pick is feasible.  acquire.select_system_host is its statement: on integer
        data every field is its bits; with infinite limits every field is ``acquire_select``'s.  Launches as for
        ``acquire_select``."""
        s, widths, flat, E, lo, hi = self._acquire_system_arguments('acquire_system_select', slots, betas, lo, hi)
        incumbent = np.ascontiguousarray(np.reshape(incumbent, -1), dtype=np.float64)
        if incumbent.shape[0] != E:
            raise ValueError("acquire_system_select: one incumbent per row of betas")
        if criterion not in ACQUIRE_INSTANCES[1:]:
            raise ValueError(f"acquire_system_select: criterion must be one of {ACQUIRE_INSTANCES[1:]}")
        picks, trace_pick = int(picks), int(trace_pick)
        rows = max(picks, 0)
        index, tiles, feasible = (np.empty(rows, dtype=np.int64) for _ in range(3))
        gain, after = np.empty(rows), np.empty(E)
        trace_g = np.empty(self.n, dtype=np.float64) if trace_pick >= 0 else None
        trace_eval = np.empty(-(-self.n // 16), dtype=np.uint8) if trace_pick >= 0 and lazy else None
        self._ck(self._lib.fokl_acquire_system_select(self._h, _ptr(s), _ptr(widths), len(widths) - 1, _ptr(flat), E,
                                                      _ptr(incumbent), _ptr(lo), _ptr(hi), ACQUIRE_INSTANCES.index(criterion),
                                                      int(bool(lazy)), picks, int(grid_cap), trace_pick, _ptr(index), _ptr(gain),
                                                      _ptr(after), _ptr(tiles), _ptr(feasible), _ptr(trace_g), _ptr(trace_eval)))
        return dict(index=index, gain=gain, incumbent_after=after, tiles_evaluated=tiles, feasible=feasible, trace_g=trace_g,
                    trace_eval=trace_eval)

    def acquire_system_incumbent(self, slots, betas, lo, hi, grid_cap=0):
        """fokl_acquire_system_incumbent over the uploaded rows (the measured points), arguments as for
        ``acquire_system_select`` -> (best [E]: per draw the largest objective over the rows feasible in that draw, -inf with
        none, NaN where a feasible row's value is not finite; count [E] int64: the feasible rows).
        acquire.incumbent_system_host is its statement.  The same arguments give the same bits whatever ``grid_cap``."""
        s, widths, flat, E, lo, hi = self._acquire_system_arguments('acquire_system_incumbent', slots, betas, lo, hi)
        best, count = np.empty(E), np.empty(E, dtype=np.int64)
        self._ck(self._lib.fokl_acquire_system_incumbent(self._h, _ptr(s), _ptr(widths), len(widths) - 1, _ptr(flat), E, _ptr(lo),
                                                         _ptr(hi), int(grid_cap), _ptr(best), _ptr(count)))
        return best, count

    def acquire_system_report(self):
        """What the last ``acquire_system_select`` or ``acquire_system_incumbent`` on this context ran
        (fokl_acquire_system_report): ``instance`` ('ei', 'pi', 'incumbent'), ``lazy``, ``constraints`` (K), the ``grid`` of
        one-wavefront workgroups over ``row_tiles`` 16-row tiles and its ``lds_bytes``, the ``bound_grid`` (of the merge
        after 'incumbent'), ``draw_group`` (draws per block of the product), ``picks``, ``launches``, ``tiles_evaluated``,
        ``tiles_evaluated_max_lazy``, ``kernel_us`` of the whole queue; ``pass_us``, ``bound_us`` and ``pivot_us`` of a
        selection are measured while the context's timing is enabled (else 0), after 'incumbent' the first two hold its two
        kernels.  'none' and zeros after a refused call."""
        out = np.zeros(16, dtype=np.int64)
        self._ck(self._lib.fokl_acquire_system_report(self._h, _ptr(out)))
        v = [int(x) for x in out]
        return dict(instance=ACQUIRE_SYSTEM_INSTANCES[v[0]], lazy=bool(v[1]), constraints=v[2], grid=v[3], bound_grid=v[4],
                    row_tiles=v[5], lds_bytes=v[6], draw_group=v[7], picks=v[8], launches=v[9], tiles_evaluated=v[10],
                    tiles_evaluated_max_lazy=v[11], kernel_us=v[12], pass_us=v[13], bound_us=v[14], pivot_us=v[15])

    def drawbest_rows(self, slots, betas, mask=None, ranks=1, grid_cap=0):
        """fokl_drawbest_rows over the uploaded rows (the pool): for every row of ``betas`` [E, nc] (a draw) its best
        ``ranks`` rows, f_sd = x_s . beta_d, sense 'max' -> dict(index [ranks, E] int64, value [ranks, E]).  ``mask`` [S]:
        rows that are no candidates where non-zero (None: none).  A NaN f never ranks, +-inf compare as numbers; value
        descending, on equal values the lower row; a draw with fewer than r + 1 candidates has index -1 and value -inf from
        rank r on.  pooloptimum.ranks_host is its statement: on integer data both fields are its bits.
        ``report['launches']`` is 2 * ranks (one pass over the pool and one merge per rank); nothing waits on the host
        between them.  At most ``DRAWBEST_MAX_COLUMNS`` columns and ``DRAWBEST_MAX_RANKS`` ranks.  ``grid_cap``: 0 the
        device's row chunks; a test hook.  The same arguments give the same bits whatever the grid."""
        s = np.ascontiguousarray(slots, dtype=np.int32)
        nc = s.shape[0]
        betas = np.ascontiguousarray(betas, dtype=np.float64)
        if betas.ndim != 2 or betas.shape[1] != nc:
            raise ValueError("betas columns must match the slot list")
        E = betas.shape[0]
        if mask is not None:
            mask = np.ascontiguousarray(np.reshape(mask, -1) != 0, dtype=np.uint8)
            if mask.shape[0] != self.n:
                raise ValueError("drawbest_rows: one mask entry per uploaded row")
        ranks = int(ranks)
        rows = max(ranks, 0)
        index, value = np.empty((rows, E), dtype=np.int64), np.empty((rows, E))
        self._ck(self._lib.fokl_drawbest_rows(self._h, _ptr(s), nc, _ptr(betas), E, _ptr(mask), ranks, int(grid_cap),
                                              _ptr(index), _ptr(value)))
        return dict(index=index, value=value)

    def drawbest_report(self):
        """What the last ``drawbest_rows`` on this context ran (fokl_drawbest_report): ``instance`` ('ran'), ``ranks``,
        ``row_tiles`` 16-row tiles in ``row_chunks`` chunks of ``tiles_per_chunk``, ``draw_blocks`` of 128 draws, the ``grid``
        of the pass kernel (row chunks rounded up to 8, times draw blocks) and the ``merge_grid``, ``lds_bytes``,
        ``coefficients`` ('registers': at most 128 columns; 'table'), the ``launches`` in all (2 * ranks), ``kernel_us`` of
        the whole queue; ``pass_us`` and ``merge_us`` are measured while the context's timing is enabled (else 0).  'none'
        and zeros after a refused call."""
        out = np.zeros(14, dtype=np.int64)
        self._ck(self._lib.fokl_drawbest_report(self._h, _ptr(out)))
        v = [int(x) for x in out]
        return dict(instance=DRAWBEST_INSTANCES[v[0]], ranks=v[1], row_tiles=v[2], row_chunks=v[3], draw_blocks=v[4], grid=v[5],
                    merge_grid=v[6], lds_bytes=v[7], coefficients=POPULATION_COEFFICIENTS[v[8]], launches=v[9],
                    tiles_per_chunk=v[10], kernel_us=v[11], pass_us=v[12], merge_us=v[13])

    def infer_inputs(self, mtx_u, betas, h, table, lo, hi, prior_mean, prior_prec, y, known_prod, starts, burnin, draws,
                     thin, jump_every, seed, draw_ids=None, rows=True, term_cap=0):
        """fokl_infer_inputs (infer.infer_inputs assembles the arguments, all in normalised coordinates): mtx_u int32
        [terms, d] the unknown columns of the interaction matrix, betas [E, terms + 1], h [E] = 0.5 / sigma^2, table
        [n_basis, width], lo / hi / prior_mean / prior_prec [d], y [K], known_prod [K, terms + 1], starts [64, d] ->
        (x [E, kept, 64, d], lp [E, kept, 64] -- both None without ``rows`` --, sums [E, 64, 2, 2, d], accepted [E, 64, 2],
        evaluations [E]): what ``infer.sample_host`` returns.  ``draw_ids`` [E]: the stream of each ensemble (default its
        index).  ``term_cap``: 0 the default launch bound; a test hook.  Needs no uploaded dataset and leaves one alone."""
        f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64)
        mtx_u = np.ascontiguousarray(mtx_u, dtype=np.int32)
        betas, h, table, lo, hi, prior_mean, prior_prec, y, known_prod, starts = (
            f64(a) for a in (betas, h, table, lo, hi, prior_mean, prior_prec, y, known_prod, starts))
        if mtx_u.ndim != 2 or betas.ndim != 2 or table.ndim != 2 or y.ndim != 1 or starts.ndim != 2 or lo.ndim != 1:
            raise ValueError("infer_inputs: array shapes disagree")
        n_terms, d = mtx_u.shape
        E, K = betas.shape[0], y.shape[0]
        if betas.shape[1] != n_terms + 1 or h.shape != (E,) or known_prod.shape != (K, n_terms + 1) or \
                starts.shape != (INFER_WALKERS, d) or any(a.shape != (d,) for a in (lo, hi, prior_mean, prior_prec)):
            raise ValueError("infer_inputs: array shapes disagree")
        ids = None
        if draw_ids is not None:
            ids = np.ascontiguousarray(draw_ids, dtype=np.uint32)
            if ids.shape != (E,):
                raise ValueError("infer_inputs: one draw id per row of betas")
        kept = -(-int(draws) // int(thin)) if int(thin) >= 1 and int(draws) >= 1 else 0
        x = np.empty((E, kept, INFER_WALKERS, d), dtype=np.float64) if rows else None
        lp = np.empty((E, kept, INFER_WALKERS), dtype=np.float64) if rows else None
        sums = np.empty((E, INFER_WALKERS, 2, 2, d), dtype=np.float64)
        accepted = np.empty((E, INFER_WALKERS, 2), dtype=np.int32)
        evaluations = np.empty(E, dtype=np.int64)
        self._ck(self._lib.fokl_infer_inputs(
            self._h, int(d), int(n_terms), _ptr(mtx_u), int(E), _ptr(betas), _ptr(h), _ptr(ids), _ptr(table),
            int(table.shape[0]), int(table.shape[1]), _ptr(lo), _ptr(hi), _ptr(prior_mean), _ptr(prior_prec), int(K), _ptr(y),
            _ptr(known_prod), _ptr(starts), int(burnin), int(draws), int(thin), int(jump_every), int(seed) & 0xFFFFFFFF,
            int(term_cap), _ptr(x), _ptr(lp), _ptr(sums), _ptr(accepted), _ptr(evaluations)))
        return x, lp, sums, accepted, evaluations

    def infer_report(self):
        """What the last ``infer_inputs`` on this context ran (fokl_infer_report): the lane ``mapping`` ('walker_per_lane': one
        draw per wavefront, lane = walker), ``lds_rows`` per lane and ``lds_bytes``, the ``grid`` of the largest launch, the
        ``launches`` of ``draws_per_launch`` ensembles, ``kernel_us`` over all of them, the ``iterations`` of a chain and the
        target ``evaluations`` in all.  'none' and zeros after a refused call."""
        out = np.zeros(9, dtype=np.int64)
        self._ck(self._lib.fokl_infer_report(self._h, _ptr(out)))
        v = [int(x) for x in out]
        return dict(mapping=INFER_MAPPINGS[v[0]], lds_rows=v[1], grid=v[2], launches=v[3], kernel_us=v[4], iterations=v[5],
                    evaluations=v[6], draws_per_launch=v[7], lds_bytes=v[8])

    def _fit_report(self, which, count):
        out = np.zeros(count, dtype=np.int64)
        self._ck(self._lib.fokl_fit_report(self._h, which, _ptr(out), count))
        return [int(v) for v in out]

    def gram_report(self):
        """What the last ``gram`` / ``gram_launch`` on this context ran (fokl_fit_report): ``kernel`` ('valu', 'tiles' = the
        k-split teams of gram_tiles_kernel, 'dma' = gram_tiles_dma_kernel; development builds also 'panel', 'tiles4'), its
        template arguments ``nt8`` (tiles per wavefront), ``half``, ``loaders``, ``lds_buffers``, ``ks``, ``depth``, the
        ``rows_per_chunk``, the plan's ``groups``, ``ct``, ``nt``, the LDS-DMA ``pieces`` and ``lds_bytes``, the row cut ``S``
        and the ``chunks_per_workgroup`` of the busiest workgroup (above 1: its chunk loop went round), ``nr_pad``,
        ``nc_pad``, the ``slabs`` reduced ``reduce_epb`` elements per block, ``row_tiles``, ``col_tiles`` and the ``lanes``
        per workgroup.  'none' and zeros after a refused call."""
        keys = ('kernel', 'nt8', 'half', 'loaders', 'lds_buffers', 'ks', 'depth', 'rows_per_chunk', 'groups', 'ct', 'nt',
                'pieces', 'lds_bytes', 'S', 'chunks_per_workgroup', 'nr_pad', 'nc_pad', 'slabs', 'reduce_epb', 'row_tiles',
                'col_tiles', 'lanes')
        ran = dict(zip(keys, self._fit_report(0, len(keys))))
        ran['kernel'], ran['half'] = GRAM_KERNELS[ran['kernel']], bool(ran['half'])
        return ran

    def resid_report(self):
        """What the last residual pass launched on this context ran: ``kernel`` ('columns' = resid_kernel over stored
        columns, 'matrix_free'), ``columns`` (matrix-free: terms), ``batches`` of 256 columns (above 1: the column table
        is reloaded per row tile), ``grid`` workgroups over ``row_tiles`` tiles of 512 rows (more tiles than workgroups:
        the tile loop went round), and the matrix-free ``layout`` (inputs x orders per input), ``order_class``, ``inputs``.
        'none' and zeros after a refused launch."""
        v = self._fit_report(1, 9)
        return dict(kernel=RESID_KERNELS[v[0]], columns=v[1], batches=v[2], grid=v[3], row_tiles=v[4], layout=(v[5], v[6]),
                    order_class=v[7], inputs=v[8])

    def basis_report(self):
        """What the last ``build_terms`` / ``build_terms_deriv`` on this context ran: the ``launches`` it split into, how
        many of them took the ``lds_table`` kernel, and ``first``, ``last``, ``last_lds`` = dict(kernel ('reg_table',
        'lds_table'), splines, lanes, factors, slabs, grid, row_tiles) of those launches ('none' and zeros where there was
        none).  Zero launches after a refused call."""
        v = self._fit_report(2, 23)
        keys = ('kernel', 'splines', 'lanes', 'factors', 'slabs', 'grid', 'row_tiles')

        def one(rec):
            d = dict(zip(keys, rec))
            d['kernel'], d['splines'] = BASIS_KERNELS[d['kernel']], bool(d['splines'])
            return d
        return dict(launches=v[0], lds_table=v[1], first=one(v[2:9]), last=one(v[9:16]), last_lds=one(v[16:23]))

    def gp_integrate_ensemble(self, n_members, n_states, n_other, n_steps, betas, per_member, mtx, rows, cols, sources,
                              n_src, forcing, norms, table, n_basis, width, h, y0, cut=None, want_members=False):
        """fokl_gp_integrate_ensemble (GP_Integrate.GP_Integrate_ensemble assembles the arguments): betas / mtx / sources
        are ctypes pointer arrays, the rest numpy; -> (mean [n_states, n_steps + 1], bounds [..., 2] or None if cut is
        None, members [n_members, n_states, n_steps + 1] or None).  Needs no uploaded dataset and leaves one alone."""
        mean = np.empty((n_states, n_steps + 1), dtype=np.float64)
        bounds = np.empty((n_states, n_steps + 1, 2), dtype=np.float64) if cut is not None else None
        members = np.empty((n_members, n_states, n_steps + 1), dtype=np.float64) if want_members else None
        self._ck(self._lib.fokl_gp_integrate_ensemble(
            self._h, int(n_members), int(n_states), int(n_other), int(n_steps), betas, _ptr(per_member), mtx, _ptr(rows),
            _ptr(cols), sources, _ptr(n_src), _ptr(forcing), _ptr(norms), _ptr(table), int(n_basis), int(width), float(h),
            _ptr(y0), int(y0.ndim == 2), int(cut or 0), _ptr(mean), _ptr(bounds), _ptr(members)))
        return mean, bounds, members

    def gp_integrate_report(self):
        """What the last ``gp_integrate_ensemble`` on this context ran (fokl_gp_integrate_report; host values, no launch):
        ``NS`` (the kernel instance = states), ``members``, ``workgroups`` (= wavefronts = ceil(members / 64)), ``lds_bytes``
        of the integration kernel, its ``launches`` and ``steps_per_launch``, ``band_lds_bytes`` (the band kernel's sorted
        list, 0 without bounds), ``band_rows`` and ``band_workgroups`` of the first launch (fewer workgroups than rows: a
        workgroup goes round the grid) and the device's ``compute_units``.  Zeros after a refused call."""
        out = np.zeros(10, dtype=np.int64)
        self._ck(self._lib.fokl_gp_integrate_report(self._h, _ptr(out)))
        keys = ('NS', 'members', 'workgroups', 'lds_bytes', 'launches', 'steps_per_launch', 'band_lds_bytes', 'band_rows',
                'band_workgroups', 'compute_units')
        return dict(zip(keys, (int(v) for v in out)))

    def simulate_ensemble(self, p):
        """fokl_simulate_ensemble for a system prepared by ``dynamics._prepare`` -> (mean [n_states, P], bounds
        [n_states, P, 2] or None, members [E, n_states, P] or None, first_saturation [E] int32).  Needs no uploaded
        dataset and leaves one alone."""
        K, E, P = int(p['K']), int(p['E']), int(p['n_steps']) + 1
        mean = np.empty((K, P), dtype=np.float64)
        bounds = np.empty((K, P, 2), dtype=np.float64) if p['want_bounds'] else None
        members = np.empty((E, K, P), dtype=np.float64) if p['want_members'] else None
        first = np.empty(E, dtype=np.int32)
        system, held = _system_struct(p, 'simulate_ensemble', coef_by_draw=False)
        self._ck(self._lib.fokl_simulate_ensemble(self._h, ctypes.byref(system), int(p['cut']) if p['want_bounds'] else 0,
                                                  _ptr(mean), _ptr(bounds), _ptr(members), _ptr(first)))
        del held
        return mean, bounds, members, first

    def simulate_report(self):
        """What the last ``simulate_ensemble`` on this context ran (fokl_simulate_report; host values, no launch): ``NS``
        (the kernel instance = states), ``members``, ``workgroups`` (= wavefronts = ceil(members / 64)), ``lds_bytes``,
        ``launches`` of the integration kernel, ``spline_factors``, ``bernoulli_factors`` and ``steps_per_launch``.  Zeros
        after a refused call."""
        out = np.zeros(8, dtype=np.int64)
        self._ck(self._lib.fokl_simulate_report(self._h, _ptr(out)))
        keys = ('NS', 'members', 'workgroups', 'lds_bytes', 'launches', 'spline_factors', 'bernoulli_factors',
                'steps_per_launch')
        return dict(zip(keys, (int(v) for v in out)))

    def simulate_adaptive(self, p):
        """fokl_simulate_adaptive for a system prepared by ``dynamics._prepare_adaptive`` -> (mean [n_states, P], bounds
        [n_states, P, 2] or None, members [E, n_states, P] or None, first_saturation [E] int32, pairs [E] int64, rejected [E]
        int64, max_level [E] int32, error [E], first_unresolved [E] int32, levels [E, steps] int8 or None).  Needs no
        uploaded dataset and leaves one alone."""
        K, E, P = int(p['K']), int(p['E']), int(p['n_steps']) + 1
        mean = np.empty((K, P), dtype=np.float64)
        bounds = np.empty((K, P, 2), dtype=np.float64) if p['want_bounds'] else None
        members = np.empty((E, K, P), dtype=np.float64) if p['want_members'] else None
        first, unresolved, max_level = (np.empty(E, dtype=np.int32) for _ in range(3))
        pairs, rejected, error = np.empty(E, dtype=np.int64), np.empty(E, dtype=np.int64), np.empty(E, dtype=np.float64)
        levels = np.zeros((E, P - 1), dtype=np.int8) if p['want_levels'] else None
        system, held = _system_struct(p, 'simulate_adaptive', coef_by_draw=False)
        atol = _f64(p['atol'])
        if atol.shape != (K,):
            raise ValueError("simulate_adaptive: array shapes disagree")
        self._ck(self._lib.fokl_simulate_adaptive(
            self._h, ctypes.byref(system), int(p['cut']) if p['want_bounds'] else 0, float(p['rtol']), _ptr(atol),
            int(p['min_halvings']), int(p['max_halvings']), _ptr(mean), _ptr(bounds), _ptr(members), _ptr(first), _ptr(pairs),
            _ptr(rejected), _ptr(max_level), _ptr(error), _ptr(unresolved), _ptr(levels)))
        del held
        return mean, bounds, members, first, pairs, rejected, max_level, error, unresolved, levels

    def simulate_adaptive_report(self):
        """What the last ``simulate_adaptive`` on this context ran (fokl_simulate_adaptive_report; host values, no launch):
        ``NS`` (the kernel instance = states), ``members``, ``workgroups`` (= wavefronts = ceil(members / 64)), ``launches``
        of the integration kernel, ``steps_per_launch``, ``lds_bytes``, ``spline_factors``, ``bernoulli_factors``,
        ``min_halvings``, ``max_halvings`` and the totals ``pairs`` and ``rejected`` over the members.  Zeros after a
        refused call."""
        out = np.zeros(12, dtype=np.int64)
        self._ck(self._lib.fokl_simulate_adaptive_report(self._h, _ptr(out)))
        keys = ('NS', 'members', 'workgroups', 'launches', 'steps_per_launch', 'lds_bytes', 'spline_factors',
                'bernoulli_factors', 'min_halvings', 'max_halvings', 'pairs', 'rejected')
        return dict(zip(keys, (int(v) for v in out)))

    def simulate_stiff(self, p):
        """fokl_simulate_stiff for a system prepared by ``dynamics._prepare_stiff`` -> (mean [n_states, P], bounds
        [n_states, P, 2] or None, members [E, n_states, P] or None, first_saturation [E] int32, steps [E] int64, rejected [E]
        int64, swaps [E] int64, max_level [E] int32, error [E], first_unresolved [E] int32, levels [E, steps] int8 or None).
        Needs no uploaded dataset and leaves one alone."""
        K, E, P = int(p['K']), int(p['E']), int(p['n_steps']) + 1
        mean = np.empty((K, P), dtype=np.float64)
        bounds = np.empty((K, P, 2), dtype=np.float64) if p['want_bounds'] else None
        members = np.empty((E, K, P), dtype=np.float64) if p['want_members'] else None
        first, unresolved, max_level = (np.empty(E, dtype=np.int32) for _ in range(3))
        steps, rejected, swaps = (np.empty(E, dtype=np.int64) for _ in range(3))
        error = np.empty(E, dtype=np.float64)
        levels = np.zeros((E, P - 1), dtype=np.int8) if p['want_levels'] else None
        system, held = _system_struct(p, 'simulate_stiff', coef_by_draw=False)
        atol = _f64(p['atol'])
        if atol.shape != (K,):
            raise ValueError("simulate_stiff: array shapes disagree")
        self._ck(self._lib.fokl_simulate_stiff(
            self._h, ctypes.byref(system), int(p['cut']) if p['want_bounds'] else 0, float(p['rtol']), _ptr(atol),
            int(p['min_halvings']), int(p['max_halvings']), _ptr(mean), _ptr(bounds), _ptr(members), _ptr(first), _ptr(steps),
            _ptr(rejected), _ptr(swaps), _ptr(max_level), _ptr(error), _ptr(unresolved), _ptr(levels)))
        del held
        return mean, bounds, members, first, steps, rejected, swaps, max_level, error, unresolved, levels

    def simulate_stiff_report(self):
        """What the last ``simulate_stiff`` on this context ran (fokl_simulate_stiff_report; host values, no launch): ``NS``
        (the kernel instance = states), ``members``, ``workgroups`` (= wavefronts = ceil(members / 64)), ``launches`` of the
        integration kernel, ``steps_per_launch`` (output steps), ``lds_bytes``, ``min_halvings``, ``max_halvings`` and the
        totals ``steps``, ``rejected`` and ``swaps`` over the members.  Zeros after a refused call."""
        out = np.zeros(11, dtype=np.int64)
        self._ck(self._lib.fokl_simulate_stiff_report(self._h, _ptr(out)))
        keys = ('NS', 'members', 'workgroups', 'launches', 'steps_per_launch', 'lds_bytes', 'min_halvings', 'max_halvings',
                'steps', 'rejected', 'swaps')
        return dict(zip(keys, (int(v) for v in out)))

    def steady_states(self, p):
        """fokl_steady_states for a system prepared by ``dynamics._prepare_steady`` -> (y [Q, E S, n_states], residual [Q, E S],
        iterations [Q, E S] int32, status [Q, E S] int8, halvings [Q, E S] int32, on_wall [Q, E S, n_states] bool, jacobian
        [Q, E S, n_states, n_states]); member e S + s is draw e from start s, so a draw's coefficients are repeated per start.
        Needs no uploaded dataset and leaves one alone."""
        K, E, S, Q = int(p['K']), int(p['E']), int(p['S']), int(p['Q'])
        M = E * S
        starts, ftol = _f64(p['starts']), _f64(p['ftol'])
        if starts.shape != (S, K) or ftol.shape != (K,) or int(p['n_steps']) != Q:
            raise ValueError("steady_states: array shapes disagree")
        members = dict(p, E=M, coef=np.repeat(_f64(p['coef']), S, axis=1), y0=np.tile(starts.T, (1, E)))
        system, held = _system_struct(members, 'steady_states', coef_by_draw=False)
        y, residual = np.empty((Q, M, K), dtype=np.float64), np.empty((Q, M), dtype=np.float64)
        iterations, halvings = np.empty((Q, M), dtype=np.int32), np.empty((Q, M), dtype=np.int32)
        status, on_wall = np.empty((Q, M), dtype=np.int8), np.empty((Q, M, K), dtype=np.uint8)
        jacobian = np.empty((Q, M, K, K), dtype=np.float64)
        self._ck(self._lib.fokl_steady_states(self._h, ctypes.byref(system), _ptr(ftol), int(p['max_iter']), int(p['max_halvings']),
                                              _ptr(y), _ptr(residual), _ptr(iterations), _ptr(status), _ptr(halvings),
                                              _ptr(on_wall), _ptr(jacobian)))
        del held
        return y, residual, iterations, status, halvings, on_wall.astype(bool), jacobian

    def steady_report(self):
        """What the last ``steady_states`` on this context ran (fokl_steady_report; host values, no launch): ``NS`` (the kernel
        instance = states), ``members`` (draws x starts), ``workgroups`` (= wavefronts = ceil(members / 64) x points),
        ``lds_bytes``, ``launches``, ``points`` and the totals ``iterations`` and ``halvings`` over the members.  Zeros after a
        refused call."""
        out = np.zeros(8, dtype=np.int64)
        self._ck(self._lib.fokl_steady_report(self._h, _ptr(out)))
        keys = ('NS', 'members', 'workgroups', 'lds_bytes', 'launches', 'points', 'iterations', 'halvings')
        return dict(zip(keys, (int(v) for v in out)))

    def assimilate_ensemble(self, p):
        """fokl_assimilate_ensemble for a system prepared by ``dynamics._prepare`` with the filter's entries added by
        ``dynamics._prepare_assimilate`` -> (stats [E, n_obs, 2 n_states + 3], particles [E, n_obs, 64, n_states] or None,
        weights [E, n_obs, 64] or None, first_saturation [E] int32, collapsed [E] int32).  Needs no uploaded dataset and
        leaves one alone."""
        K, E, P = int(p['K']), int(p['E']), int(p['n_steps']) + 1
        system, held = _system_struct(p, 'assimilate_ensemble', coef_by_draw=True)
        ids = np.ascontiguousarray(p['draw_ids'], dtype=np.uint32)
        obs_state, obs_sd, obs_row = _i32(p['obs_state']), _f64(p['obs_sd']), _i32(p['obs_row'])
        data, obs_const, q, y0_sd = _f64(p['data']), _f64(p['obs_const']), _f64(p['process_q']), _f64(p['y0_sd'])
        n_obs = data.shape[0] if data.ndim == 2 else -1
        if ids.shape != (E,) or obs_state.ndim != 1 or obs_sd.shape != obs_state.shape or data.ndim != 2 or \
                data.shape[1] != obs_state.shape[0] or obs_row.shape != (P,) or obs_const.shape != (n_obs,) or \
                q.shape != (K,) or y0_sd.shape != (K,):
            raise ValueError("assimilate_ensemble: array shapes disagree")
        stats = np.empty((E, n_obs, 2 * K + 3), dtype=np.float64)
        keep = bool(p['want_particles'])
        particles = np.empty((E, n_obs, ASSIMILATE_PARTICLES, K), dtype=np.float64) if keep else None
        weights = np.empty((E, n_obs, ASSIMILATE_PARTICLES), dtype=np.float64) if keep else None
        first, collapsed = np.empty(E, dtype=np.int32), np.empty(E, dtype=np.int32)
        self._ck(self._lib.fokl_assimilate_ensemble(
            self._h, ctypes.byref(system), _ptr(ids), obs_state.shape[0], _ptr(obs_state), _ptr(obs_sd), n_obs, _ptr(obs_row),
            _ptr(data), _ptr(obs_const), _ptr(q), _ptr(y0_sd), float(p['threshold']), int(p['seed']) & 0xFFFFFFFF, _ptr(stats),
            _ptr(particles), _ptr(weights), _ptr(first), _ptr(collapsed)))
        del held
        return stats, particles, weights, first, collapsed

    def assimilate_report(self):
        """What the last ``assimilate_ensemble`` on this context ran (fokl_assimilate_report; host values, no launch): ``NS``
        (the kernel instance = states), ``draws``, ``grid`` (workgroups = wavefronts = draws), ``lds_bytes``, ``launches``
        of ``steps_per_launch`` steps, ``observations``, ``spline_factors`` and ``bernoulli_factors``.  Zeros after a
        refused call."""
        out = np.zeros(9, dtype=np.int64)
        self._ck(self._lib.fokl_assimilate_report(self._h, _ptr(out)))
        keys = ('NS', 'draws', 'grid', 'lds_bytes', 'launches', 'steps_per_launch', 'observations', 'spline_factors',
                'bernoulli_factors')
        return dict(zip(keys, (int(v) for v in out)))

    def calibrate(self, p):
        """fokl_calibrate_ensemble for a system prepared by ``dynamics._prepare_calibrate`` -> (x [E, kept, 128, d] or None, lp
        [E, kept, 128] or None, saturated [E, kept, 128] bool or None, sums [E, 128, 2, 2, d], accepted [E, 128, 2] int32,
        evaluations [E] int64, invalid [E] bool, trajectories [E, 128, n_states, P] or None).  Needs no uploaded dataset and
        leaves one alone."""
        K, E, P, d = int(p['K']), int(p['E']), int(p['n_steps']) + 1, int(p['d'])
        system, held = _system_struct(p, 'calibrate', coef_by_draw=True)
        problem, held_problem = _calibrate_problem_struct(p, 'calibrate')
        kept = -(-int(p['draws_kept']) // max(int(p['thin']), 1))
        rows = bool(p['want_rows'])
        x = np.empty((E, kept, CALIBRATE_WALKERS, d), dtype=np.float64) if rows else None
        lp = np.empty((E, kept, CALIBRATE_WALKERS), dtype=np.float64) if rows else None
        sat = np.empty((E, kept, CALIBRATE_WALKERS), dtype=np.int32) if rows else None
        sums = np.empty((E, CALIBRATE_WALKERS, 2, 2, d), dtype=np.float64)
        accepted = np.empty((E, CALIBRATE_WALKERS, 2), dtype=np.int32)
        evaluations, invalid = np.empty(E, dtype=np.int64), np.empty(E, dtype=np.int32)
        trajectories = np.empty((E, CALIBRATE_WALKERS, K, P), dtype=np.float64) if p['want_trajectories'] else None
        self._ck(self._lib.fokl_calibrate_ensemble(
            self._h, ctypes.byref(system), ctypes.byref(problem), _ptr(x), _ptr(lp), _ptr(sat), _ptr(sums), _ptr(accepted),
            _ptr(evaluations), _ptr(invalid), _ptr(trajectories)))
        del held, held_problem
        return x, lp, (sat != 0 if rows else None), sums, accepted, evaluations, invalid != 0, trajectories

    def calibrate_report(self):
        """What the last ``calibrate`` on this context ran (fokl_calibrate_report; host values, no launch): ``NS`` (the kernel
        instance = states), ``draws`` (= workgroups = wavefronts), ``lds_bytes``, ``launches`` (the replay of the final
        ensemble included) of ``iterations_per_launch`` iterations, ``evaluations`` (trajectories integrated, all draws),
        ``kernel_us`` and ``iterations``.  Zeros after a refused call."""
        out = np.zeros(8, dtype=np.int64)
        self._ck(self._lib.fokl_calibrate_report(self._h, _ptr(out)))
        keys = ('NS', 'draws', 'lds_bytes', 'launches', 'iterations_per_launch', 'evaluations', 'kernel_us', 'iterations')
        return dict(zip(keys, (int(v) for v in out)))

    def control_solve(self, p):
        """fokl_control_solve for a system prepared by ``dynamics._prepare_control`` -> (solved, best_start [E] int32,
        members [E, n_states, P], first_saturation [E] int32); ``solved`` holds z [E, S, D], cost, cost_start, status,
        iterations, descent_steps [E, S] and, for max_iter == 0, ``first_pass`` (F [E, S], g [E, S, D], H [E, S, D, D]).  Needs no uploaded
        dataset and leaves one alone."""
        K, E, P, S, D = int(p['K']), int(p['E']), int(p['n_steps']) + 1, int(p['starts']), int(p['D'])
        system, held = _system_struct(p, 'control_solve', coef_by_draw=True)
        problem, held_problem = _control_problem_struct(p, 'control_solve')
        z = np.empty((E, S, D), dtype=np.float64)
        cost, cost_start = np.empty((E, S), dtype=np.float64), np.empty((E, S), dtype=np.float64)
        status, iterations = np.empty((E, S), dtype=np.int32), np.empty((E, S), dtype=np.int32)
        descent = np.empty((E, S), dtype=np.int32)
        best, first = np.empty(E, dtype=np.int32), np.empty(E, dtype=np.int32)
        members = np.empty((E, K, P), dtype=np.float64)
        want_first = int(p['max_iter']) == 0
        fF = np.empty((E, S), dtype=np.float64) if want_first else None
        fg = np.empty((E, S, D), dtype=np.float64) if want_first else None
        fH = np.empty((E, S, D, D), dtype=np.float64) if want_first else None
        self._ck(self._lib.fokl_control_solve(
            self._h, ctypes.byref(system), ctypes.byref(problem), _ptr(z), _ptr(cost), _ptr(cost_start), _ptr(status),
            _ptr(iterations), _ptr(descent), _ptr(best), _ptr(members), _ptr(first), _ptr(fF), _ptr(fg), _ptr(fH)))
        del held, held_problem
        solved = dict(z=z, cost=cost, cost_start=cost_start, status=status, iterations=iterations, descent_steps=descent)
        if want_first:
            solved['first_pass'] = dict(F=fF, g=fg, H=fH)
        return solved, best, members, first

    def control_report(self):
        """What the last ``control_solve`` on this context ran (fokl_control_report; host values, no launch): ``NS`` (the
        kernel instance = states), ``solves`` (= workgroups = wavefronts), ``D``, ``lds_bytes``, ``launches_queued``,
        ``launches_with_work``, ``spline_factors`` and ``bernoulli_factors``.  Zeros after a refused call."""
        out = np.zeros(8, dtype=np.int64)
        self._ck(self._lib.fokl_control_report(self._h, _ptr(out)))
        keys = ('NS', 'solves', 'D', 'lds_bytes', 'launches_queued', 'launches_with_work', 'spline_factors',
                'bernoulli_factors')
        return dict(zip(keys, (int(v) for v in out)))

    def control_pooled_solve(self, p, first_trial=False):
        """fokl_control_pooled_solve for a system prepared by ``dynamics._prepare_control_pooled`` -> (solved, best_start,
        members [E, n_states, P], first_saturation [E] int32, cost_draws [E]); ``solved`` holds z [S, D], cost, cost_start,
        status, iterations, descent_steps [S] and, for max_iter == 0, ``first_pass`` (the pooled F [S], g [S, D], H [S, D, D]
        and the draws' own F_draws [S, E], g_draws [S, E, D], H_draws [S, E, D, D]; NaN for a draw of weight 0).  With
        ``first_trial=True`` ``solved`` also holds ``first_trial``: the trial half of iteration 0 as the device left it, in
        the layout of ``dynamics._control_pooled_solve_host``'s ``first_trial`` (``_first_trial_dict`` below), with
        ``Ft_chunks`` [S, chunks, 2, 31], the chunk sums the accept launch adds, and ``Ft`` their sum in chunk order formed
        here.  Needs no uploaded dataset and leaves one alone."""
        K, E, P, S, D = int(p['K']), int(p['E']), int(p['n_steps']) + 1, int(p['starts']), int(p['D'])
        system, held = _system_struct(p, 'control_pooled_solve', coef_by_draw=True)
        problem, held_problem = _control_problem_struct(p, 'control_pooled_solve')
        w = _f64(p['pool_w'])
        if w.shape != (E,):
            raise ValueError("control_pooled_solve: array shapes disagree")
        n = 2 + D + D * D
        z = np.empty((S, D), dtype=np.float64)
        cost, cost_start = np.empty(S, dtype=np.float64), np.empty(S, dtype=np.float64)
        status, iterations, descent = (np.empty(S, dtype=np.int32) for _ in range(3))
        best, first = np.empty(1, dtype=np.int32), np.empty(E, dtype=np.int32)
        members, cost_draws = np.empty((E, K, P), dtype=np.float64), np.empty(E, dtype=np.float64)
        want_first = int(p['max_iter']) == 0
        pooled = np.empty((S, n), dtype=np.float64) if want_first else None
        rows = np.empty((S, E, n), dtype=np.float64) if want_first else None
        trace = _FirstTrial(S, E, D) if first_trial else None
        self._ck(self._lib.fokl_control_pooled_solve(
            self._h, ctypes.byref(system), ctypes.byref(problem), _ptr(w), _ptr(z), _ptr(cost), _ptr(cost_start), _ptr(status),
            _ptr(iterations), _ptr(descent), _ptr(best), _ptr(members), _ptr(first), _ptr(cost_draws), _ptr(pooled), _ptr(rows),
            trace.ref() if trace else None))
        del held, held_problem
        solved = dict(z=z, cost=cost, cost_start=cost_start, status=status, iterations=iterations, descent_steps=descent)
        if trace:
            solved['first_trial'] = trace.result(pooled=True)
        if want_first:
            solved['first_pass'] = dict(F=pooled[:, 0].copy(), g=pooled[:, 2:2 + D].copy(), H=pooled[:, 2 + D:].reshape(S, D, D).copy(),
                                        F_draws=rows[:, :, 0].copy(), g_draws=rows[:, :, 2:2 + D].copy(),
                                        H_draws=rows[:, :, 2 + D:].reshape(S, E, D, D).copy())
        return solved, int(best[0]), members, first, cost_draws

    def control_pooled_report(self):
        """What the last ``control_pooled_solve`` on this context ran (fokl_control_pooled_report; host values, no launch):
        ``NS``, ``draws``, ``starts``, ``D``, ``chunks`` (of 64 draws), ``lds_bytes`` of the per-draw kernels and
        ``step_lds_bytes`` of the step kernel, ``iterations_queued``, ``iterations_with_work``, ``launches_per_iteration``
        (6) and, with kernel timing enabled, the nanoseconds spent in the launches of each kind (``tangent_ns``,
        ``chunk_ns``, ``step_ns``, ``trial_ns``, ``accept_ns``).  Zeros after a refused call."""
        out = np.zeros(15, dtype=np.int64)
        self._ck(self._lib.fokl_control_pooled_report(self._h, _ptr(out)))
        keys = ('NS', 'draws', 'starts', 'D', 'chunks', 'lds_bytes', 'step_lds_bytes', 'iterations_queued', 'iterations_with_work',
                'launches_per_iteration', 'tangent_ns', 'chunk_ns', 'step_ns', 'trial_ns', 'accept_ns')
        return dict(zip(keys, (int(v) for v in out)))

    def control_cvar_solve(self, p, first_trial=False):
        """fokl_control_cvar_solve for a system prepared as for ``control_pooled_solve`` with ``alpha``, ``smoothing`` and
        ``epsilon`` (None: relative) -> what ``control_pooled_solve`` returns, ``solved`` also holding ``epsilon`` (as used)
        and, for max_iter == 0, ``first_pass``: phi, a [S], g [S, D], H [S, D, D], q, c [S, E] and the draws' own F_draws,
        g_draws, H_draws -- for alpha == 0 ``control_pooled_solve``'s.  With ``first_trial=True`` ``solved`` also holds
        ``first_trial`` in the layout of ``dynamics._control_cvar_solve_host``'s: ``phi_t`` and ``a_t`` [S, 2, 31] of the
        trial-side risk launch in place of the pooled ``Ft`` (for alpha == 0 ``control_pooled_solve``'s)."""
        K, E, P, S, D = int(p['K']), int(p['E']), int(p['n_steps']) + 1, int(p['starts']), int(p['D'])
        system, held = _system_struct(p, 'control_cvar_solve', coef_by_draw=True)
        problem, held_problem = _control_problem_struct(p, 'control_cvar_solve')
        w = _f64(p['pool_w'])
        if w.shape != (E,):
            raise ValueError("control_cvar_solve: array shapes disagree")
        n = 2 + D + D * D
        alpha = float(p['alpha'])
        epsilon = float('nan') if p['epsilon'] is None else float(p['epsilon'])
        z = np.empty((S, D), dtype=np.float64)
        cost, cost_start = np.empty(S, dtype=np.float64), np.empty(S, dtype=np.float64)
        status, iterations, descent = (np.empty(S, dtype=np.int32) for _ in range(3))
        best, first = np.empty(1, dtype=np.int32), np.empty(E, dtype=np.int32)
        members, cost_draws = np.empty((E, K, P), dtype=np.float64), np.empty(E, dtype=np.float64)
        used = np.full(1, np.nan)
        want_first = int(p['max_iter']) == 0
        pooled = np.empty((S, n), dtype=np.float64) if want_first else None
        rows = np.empty((S, E, n), dtype=np.float64) if want_first else None
        fa = np.empty(S, dtype=np.float64) if want_first else None
        fq = np.empty((S, E), dtype=np.float64) if want_first else None
        fc = np.empty((S, E), dtype=np.float64) if want_first else None
        trace = _FirstTrial(S, E, D) if first_trial else None
        self._ck(self._lib.fokl_control_cvar_solve(
            self._h, ctypes.byref(system), ctypes.byref(problem), _ptr(w), alpha, float(p['smoothing']), epsilon, _ptr(z),
            _ptr(cost), _ptr(cost_start), _ptr(status), _ptr(iterations), _ptr(descent), _ptr(best), _ptr(members), _ptr(first),
            _ptr(cost_draws), _ptr(used), _ptr(pooled), _ptr(rows), _ptr(fa), _ptr(fq), _ptr(fc),
            trace.ref() if trace else None))
        del held, held_problem
        solved = dict(z=z, cost=cost, cost_start=cost_start, status=status, iterations=iterations, descent_steps=descent,
                      epsilon=float(used[0]))
        if trace:
            solved['first_trial'] = trace.result(pooled=alpha == 0)
        if want_first:
            parts = dict(g=pooled[:, 2:2 + D].copy(), H=pooled[:, 2 + D:].reshape(S, D, D).copy(), F_draws=rows[:, :, 0].copy(),
                         g_draws=rows[:, :, 2:2 + D].copy(), H_draws=rows[:, :, 2 + D:].reshape(S, E, D, D).copy())
            if alpha == 0:
                solved['first_pass'] = dict(F=pooled[:, 0].copy(), **parts)
            else:
                solved['first_pass'] = dict(phi=pooled[:, 0].copy(), a=fa, q=fq, c=fc, **parts)
        return solved, int(best[0]), members, first, cost_draws

    def control_cvar_report(self):
        """What the last ``control_cvar_solve`` with alpha > 0 on this context ran (fokl_control_cvar_report; host values, no
        launch): ``NS``, ``draws``, ``starts``, ``D``, ``chunks`` (of 64 draws), ``lds_bytes`` of the per-draw kernels,
        ``step_lds_bytes``, ``risk_lds_bytes`` and ``risk_threads`` of the risk kernel, ``iterations_queued``,
        ``iterations_with_work``, ``launches_per_iteration`` (7) and, with kernel timing enabled, the nanoseconds spent in the
        launches of each kind (``tangent_ns``, ``risk_ns``, ``chunk_ns``, ``step_ns``, ``trial_ns``, ``accept_ns``).  Zeros
        after a refused call and after alpha == 0 (``control_pooled_report`` has that call)."""
        out = np.zeros(18, dtype=np.int64)
        self._ck(self._lib.fokl_control_cvar_report(self._h, _ptr(out)))
        keys = ('NS', 'draws', 'starts', 'D', 'chunks', 'lds_bytes', 'step_lds_bytes', 'risk_lds_bytes', 'risk_threads',
                'iterations_queued', 'iterations_with_work', 'launches_per_iteration', 'tangent_ns', 'risk_ns', 'chunk_ns',
                'step_ns', 'trial_ns', 'accept_ns')
        return dict(zip(keys, (int(v) for v in out)))

    @staticmethod
    def _step_trace(rows, m, K=0, C=0):
        """The fields of a trace [E, S, stride] (fokl_hip_internal.h: fokl_model_optimize_trace) by name; flags as bool,
        counts and statuses as int64 (a status that was never written: -9)."""
        h = m * (m + 1) // 2
        flag = lambda a: np.nan_to_num(a, nan=0.0) != 0
        whole = lambda a: np.nan_to_num(a, nan=-9.0).astype(np.int64)
        out = dict(running=flag(rows[..., 0]), F=rows[..., 1], noise=rows[..., 2], pg=rows[..., 3],
                   active=(whole(rows[..., 4])[..., None] >> np.arange(m)) & 1 == 1, status_tests=whole(rows[..., 5]),
                   stepping=flag(rows[..., 6]), use_steepest=flag(rows[..., 7]), trials=whole(rows[..., 8]),
                   alpha=rows[..., 9], failed=flag(rows[..., 10]), steepest=flag(rows[..., 11]), status=whole(rows[..., 12]))
        at = 13
        for name, width in (('x_in', m), ('g', m), ('H', h), ('factor', h), ('d', m), ('Ft', OPTIMIZE_TRIALS), ('x_out', m)):
            out[name] = rows[..., at:at + width]
            at += width
        if K:
            for name, width in (('ev', K), ('nz', K), ('lam', 2 * C), ('rho', 1), ('inner', 1), ('target', 1), ('viol', 1),
                                ('measure', 1), ('update', 1), ('good', 1), ('lam_out', 2 * C), ('rho_out', 1),
                                ('inner_out', 1), ('target_out', 1)):
                out[name] = rows[..., at:at + width] if name in ('ev', 'nz', 'lam', 'lam_out') else rows[..., at]
                at += width
            out['update'], out['good'] = flag(out['update']), flag(out['good'])
        assert at == rows.shape[-1]
        return out

    def _optimize_report(self, call):
        out = np.zeros(9, dtype=np.int64)
        self._ck(call(self._h, _ptr(out)))
        keys = ('instance', 'grid', 'lds_bytes', 'lds_raised', 'slots', 'side_list', 'solves', 'launches', 'traced')
        rep = dict(zip(keys, (int(v) for v in out)))
        rep['instance'] = OPTIMIZE_INSTANCES[rep['instance']]
        return rep

    def optimize_report(self):
        """What the last ``model_optimize`` on this context ran (fokl_optimize_report; host values, no launch):
        ``instance`` ('uniform': a wavefront belongs to one draw, 'per_lane'), ``grid`` (workgroups = wavefronts),
        ``lds_bytes``, ``lds_raised`` (1: the attribute that allows more than 64 KB was set), ``slots`` (distinct (input,
        order) factors), ``side_list`` (entries), ``solves``, ``launches``, ``traced``.  'none' and zeros after a refused
        call."""
        return self._optimize_report(self._lib.fokl_optimize_report)

    def system_optimize_report(self):
        """``optimize_report`` for the last ``system_optimize`` (fokl_system_optimize_report): ``grid`` is the first
        launch's, ``slots`` the largest model's."""
        return self._optimize_report(self._lib.fokl_system_optimize_report)

    def model_optimize(self, mtx, betas, table, lo, hi, starts, sign, max_iter, tol, trace_iteration=None):
        """fokl_model_optimize (optimize.optimize assembles the arguments, all in normalised coordinates): mtx int32
        [terms, m], betas [E, terms + 1], table [n_basis, width], lo / hi [m], starts [S, m], sign +1 (minimise) or -1
        -> (x [E, S, m], model value [E, S], iterations [E, S], status [E, S]).  Needs no uploaded dataset and leaves
        one alone.  trace_iteration=k (fokl_model_optimize_trace): a fifth result, the dict of what iteration k of every
        solve saw and decided ([E, S, ...] each; ``_step_trace`` names the fields)."""
        mtx = np.ascontiguousarray(mtx, dtype=np.int32)
        betas, table, starts = (np.ascontiguousarray(a, dtype=np.float64) for a in (betas, table, starts))
        lo, hi = np.ascontiguousarray(lo, dtype=np.float64), np.ascontiguousarray(hi, dtype=np.float64)
        n_terms, m = mtx.shape
        if betas.ndim != 2 or betas.shape[1] != n_terms + 1 or starts.ndim != 2 or starts.shape[1] != m or \
                lo.shape != (m,) or hi.shape != (m,) or table.ndim != 2:
            raise ValueError("model_optimize: array shapes disagree")
        E, S = betas.shape[0], starts.shape[0]
        x = np.empty((E, S, m), dtype=np.float64)
        f = np.empty((E, S), dtype=np.float64)
        iterations = np.empty((E, S), dtype=np.int32)
        status = np.empty((E, S), dtype=np.int32)
        args = (self._h, int(m), int(n_terms), _ptr(mtx), int(E), _ptr(betas), _ptr(table), int(table.shape[0]),
                int(table.shape[1]), _ptr(lo), _ptr(hi), int(S), _ptr(starts), float(sign), int(max_iter), float(tol), _ptr(x),
                _ptr(f), _ptr(iterations), _ptr(status))
        if trace_iteration is None:
            self._ck(self._lib.fokl_model_optimize(*args))
            return x, f, iterations, status
        rows = np.empty((E, S, 13 + 4 * m + m * (m + 1) + OPTIMIZE_TRIALS), dtype=np.float64)
        self._ck(self._lib.fokl_model_optimize_trace(*args, int(trace_iteration), _ptr(rows)))
        return x, f, iterations, status, self._step_trace(rows, m)

    def system_optimize(self, p, trace_iteration=None):
        """fokl_system_optimize for a system prepared by ``optimize._prepare_system`` (common normalised coordinates)
        -> (x [E, S, n], objective [E, S], violation [E, S], model values [E, S, K], multipliers [E, S, C], iterations
        [E, S], status [E, S]): what ``optimize.solve_system_host`` returns.  Needs no uploaded dataset and leaves one
        alone.  trace_iteration=k (fokl_system_optimize_trace): one more result, the dict of what iteration k of every
        solve saw and decided (``_step_trace``)."""
        i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
        f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64)
        n, K, cons = int(p['n']), int(p['K']), p['cons']
        C = len(cons)
        n_inputs, n_terms = i32([m.shape[1] for m in p['mtxs']]), i32([m.shape[0] for m in p['mtxs']])
        mtx = i32(np.concatenate([np.asarray(m, dtype=np.int32).ravel() for m in p['mtxs']]))
        var_of = i32(np.concatenate(p['var_of']))
        shift, slope = f64(np.concatenate(p['shift'])), f64(np.concatenate(p['slope']))
        betas, table, starts, lo, hi = f64(p['coef']), f64(p['table']), f64(p['starts']), f64(p['lo']), f64(p['hi'])
        if betas.ndim != 2 or betas.shape[1] != int(n_terms.sum()) + K or starts.ndim != 2 or starts.shape[1] != n or \
                lo.shape != (n,) or hi.shape != (n,) or table.ndim != 2 or var_of.shape != shift.shape or \
                var_of.shape[0] != int(n_inputs.sum()):
            raise ValueError("system_optimize: array shapes disagree")
        con_model, con_var = i32([c['model'] for c in cons]), i32([c['var'] for c in cons])
        con_par = f64([[c['lo'], c['hi'], c['scale'], c['offset'], c['span']] for c in cons]).reshape(C, 5)
        obj_var = int(p['obj_var'])
        offset, span = (0.0, 1.0) if obj_var >= 0 else (0.0, 0.0)          # a variable objective: its normalised coordinate
        E, S = betas.shape[0], starts.shape[0]
        x = np.empty((E, S, n), dtype=np.float64)
        f, violation = np.empty((E, S), dtype=np.float64), np.empty((E, S), dtype=np.float64)
        y, mu = np.empty((E, S, K), dtype=np.float64), np.empty((E, S, C), dtype=np.float64)
        iterations, status = np.empty((E, S), dtype=np.int32), np.empty((E, S), dtype=np.int32)
        args = (self._h, n, K, _ptr(n_inputs), _ptr(n_terms), _ptr(mtx), _ptr(var_of), _ptr(shift), _ptr(slope), int(E),
                _ptr(betas), _ptr(table), int(table.shape[0]), int(table.shape[1]), _ptr(lo), _ptr(hi), int(S), _ptr(starts),
                int(p['obj_model']), obj_var, offset, span, float(p['sign']), C, _ptr(con_model), _ptr(con_var), _ptr(con_par),
                int(p['max_iter']), float(p['tol']), float(p['ctol']), _ptr(x), _ptr(f), _ptr(violation), _ptr(y), _ptr(mu),
                _ptr(iterations), _ptr(status))
        if trace_iteration is None:
            self._ck(self._lib.fokl_system_optimize(*args))
            return x, f, violation, y, mu, iterations, status
        rows = np.empty((E, S, 13 + 4 * n + n * (n + 1) + OPTIMIZE_TRIALS + 2 * K + 4 * C + 10), dtype=np.float64)
        self._ck(self._lib.fokl_system_optimize_trace(*args, int(trace_iteration), _ptr(rows)))
        return x, f, violation, y, mu, iterations, status, self._step_trace(rows, n, K, C)

    def embedded_hmc(self, n_gps, term_slots, col_slots, ops, consts, result, chains, draws, leapfrog, seed, q0=None,
                     eps0=0.0, adapt=True, want_grad0=False, want_proposal=False):
        """fokl_embedded_hmc (embedded.py assembles the arguments) over the uploaded dataset: term_slots the basis columns
        (ones first), col_slots the equation's columns, ops int32 [n_ops, 3] and consts the tape -> dict of states
        [chains, draws + 1, D], potential, accepted, eps_hist [chains, draws // 50], inv_mass, eps_final, status, mass_updated
        (and grad0 / proposal when asked for)."""
        term_slots = np.ascontiguousarray(term_slots, dtype=np.int32)
        col_slots = np.ascontiguousarray(col_slots, dtype=np.int32).reshape(-1)
        ops = np.ascontiguousarray(ops, dtype=np.int32).reshape(-1, 3)
        consts = np.ascontiguousarray(consts, dtype=np.float64).reshape(-1)
        chains, draws, n_coef = int(chains), int(draws), term_slots.shape[0]
        D = int(n_gps) * n_coef + 1
        if q0 is not None:
            q0 = np.ascontiguousarray(q0, dtype=np.float64)
            if q0.shape != (chains, D):
                raise ValueError("embedded_hmc: q0 must be [chains, D]")
        rows, wins = max(chains, 0), max(draws, 0) // 50
        out = dict(states=np.empty((rows, max(draws, 0) + 1, D)), potential=np.empty((rows, max(draws, 0) + 1)),
                   accepted=np.empty((rows, max(draws, 0) + 1), dtype=np.int32), eps_hist=np.empty((rows, wins)),
                   inv_mass=np.empty((rows, D)), eps_final=np.empty(rows), flags=np.empty((rows, 2), dtype=np.int32),
                   grad0=np.empty((rows, D)) if want_grad0 else None,
                   proposal=np.empty((rows, D + 1)) if want_proposal else None)
        self._ck(self._lib.fokl_embedded_hmc(
            self._h, int(n_gps), n_coef, _ptr(term_slots), col_slots.shape[0], _ptr(col_slots), ops.shape[0], _ptr(ops),
            consts.shape[0], _ptr(consts), int(result), chains, draws, int(leapfrog), int(seed) & 0xFFFFFFFF, _ptr(q0),
            float(eps0), int(bool(adapt)), _ptr(out['states']), _ptr(out['potential']), _ptr(out['accepted']),
            _ptr(out['eps_hist']), _ptr(out['inv_mass']), _ptr(out['eps_final']), _ptr(out['flags']), _ptr(out['grad0']),
            _ptr(out['proposal'])))
        flags = out.pop('flags')
        out['status'], out['mass_updated'] = flags[:, 0].copy(), flags[:, 1].astype(bool)
        return out

    def embedded_plan(self, n_gps, n_ops):
        """fokl_embedded_plan: the launch ``embedded_hmc`` makes for a tape of n_ops operations over n_gps GPs -> dict of
        threads (256 or 128 per workgroup) and lds_bytes (the dynamic LDS it asks for)."""
        threads, lds_bytes = c_int(0), ctypes.c_size_t(0)
        _check(self._lib.fokl_embedded_plan(int(n_gps), int(n_ops), ctypes.byref(threads), ctypes.byref(lds_bytes)))
        return dict(threads=threads.value, lds_bytes=lds_bytes.value)

    def read_slot(self, slot, row0=0, nrows=None):
        nrows = self.n - row0 if nrows is None else nrows
        out = np.empty(int(nrows), dtype=np.float64)
        self._ck(self._lib.fokl_read_slot(self._h, int(slot), int(row0), int(nrows), _ptr(out)))
        return out

    def write_slot(self, slot, values, row0=0):
        v = np.ascontiguousarray(values, dtype=np.float64)
        self._ck(self._lib.fokl_write_slot(self._h, int(slot), int(row0), v.shape[0], _ptr(v)))

    def probe(self, what):
        """Sustained rate of a trivial kernel on this device: what = 0 HBM read, 1 HBM write, 2 one read : seven
        writes (bytes/s), 3 fp64 MFMA on register operands (flop/s) -- include/fokl_hip.h: fokl_probe."""
        rate = c_dbl(0)
        self._ck(self._lib.fokl_probe(self._h, int(what), ctypes.byref(rate)))
        return rate.value

    def timing_enable(self, on=True):
        self._ck(self._lib.fokl_timing_enable(self._h, int(bool(on))))

    def timing_reset(self):
        self._ck(self._lib.fokl_timing_reset(self._h))

    def timing_get(self, kernel_id):
        ms, launches, nbytes, flops, ideal = c_dbl(0), c_i64(0), c_dbl(0), c_dbl(0), c_dbl(0)
        self._ck(self._lib.fokl_timing_get(self._h, int(kernel_id), ctypes.byref(ms), ctypes.byref(launches),
                                           ctypes.byref(nbytes), ctypes.byref(flops), ctypes.byref(ideal)))
        return dict(ms=ms.value, launches=launches.value, bytes=nbytes.value, flops=flops.value,
                    ideal_ms=ideal.value)

    def timing_get_gram(self):
        """All Gram launches: the HBM-bound ones (K_GRAM) and the fp64-MFMA-bound ones (K_GRAM_MFMA) together."""
        a, b = self.timing_get(K_GRAM), self.timing_get(K_GRAM_MFMA)
        return {key: a[key] + b[key] for key in a}

    # -- RCCL ------------------------------------------------------------------------------------------
    @staticmethod
    def comm_unique_id():
        buf = ctypes.create_string_buffer(UNIQUE_ID_BYTES)
        _check(load().fokl_comm_unique_id(buf))
        return buf.raw

    def comm_init(self, unique_id, rank, world):
        buf = ctypes.create_string_buffer(bytes(unique_id), UNIQUE_ID_BYTES)
        self._ck(self._lib.fokl_comm_init(self._h, buf, int(rank), int(world)))

    def comm_destroy(self):
        self._ck(self._lib.fokl_comm_destroy(self._h))

    @staticmethod
    def comm_init_detached(device, unique_id, rank, world):
        """ncclCommInitRank without a context (fokl_comm_init_detached) -> opaque communicator for comm_adopt."""
        buf = ctypes.create_string_buffer(bytes(unique_id), UNIQUE_ID_BYTES)
        comm = c_vp(0)
        _check(load().fokl_comm_init_detached(int(device), buf, int(rank), int(world), ctypes.byref(comm)))
        return comm

    def comm_adopt(self, comm, rank, world):
        self._ck(self._lib.fokl_comm_adopt(self._h, comm, int(rank), int(world)))

    @staticmethod
    def comm_release_detached(comm):
        load().fokl_comm_release_detached(comm)

    def allgather(self, values, world):
        v = np.ascontiguousarray(values, dtype=np.float64)
        out = np.empty((int(world), v.shape[0]), dtype=np.float64)
        self._ck(self._lib.fokl_comm_allgather_f64(self._h, _ptr(v), v.shape[0], _ptr(out)))
        return out

    def allreduce_sum(self, values):
        v = np.array(values, dtype=np.float64, copy=True)
        self._ck(self._lib.fokl_comm_allreduce_sum_f64(self._h, _ptr(v), v.size))
        return v

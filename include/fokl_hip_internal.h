/*
 * fokl_hip_internal.h -- what libfokl_hip.so exports BESIDE its C ABI (include/fokl_hip.h): the plumbing of this
 * package's own host pipeline, bound by fokl_gpy_amd/_capi.py and by nothing else.  Not part of the boundary a maintainer of
 * the reference would bind (INTEGRATION.md binds fokl_hip.h only) and free to change between releases:
 *
 *   fokl_stream_*              the numpy-legacy random stream in two phases (bulk threads + one serial walk)
 *   fokl_pool_*                the host threads of one fit (noise / chain / finish / spectral queues)
 *   fokl_search_* / fokl_outcome_* / fokl_spectrum_*
 *                              the search's per-evaluation work next to the kill-test loop (FR:1650-1690)
 *   fokl_dchain_* / fokl_dspectral_* / fokl_device_dgemm* / fokl_host_alloc
 *                              the device engines behind G3 (and the opt-in G2) and their page-locked memory
 *   fokl_gibbs_chain_segments_host
 *                              a host chain's recursion in verified segments (the boundary's header is full)
 *   fokl_model_optimize        the multistart optimiser behind fokl_gpy_amd/optimize.py (the boundary's header is full)
 *   fokl_system_optimize       its constrained counterpart over a system of models (optimize.optimize_system)
 *   fokl_model_optimize_trace / fokl_system_optimize_trace / fokl_optimize_report / fokl_system_optimize_report
 *                              one iteration of every solve as the product kernels saw it, and what they launched
 *   fokl_predict_report        which kernel the last fokl_predict call ran, over what grid, and how many of its tiles took
 *                              the exact fallback (the boundary's header is full)
 *   fokl_population_stats / fokl_population_report
 *                              a population of inputs through every posterior draw, reduced over the rows per draw
 *                              (fokl_gpy_amd/population.py), and what its last launch ran
 *   fokl_fit_report            the same for the fit's kernels: which Gram instance, residual branch and basis kernels the
 *                              last launches ran, with their launch parameters
 *   fokl_resample_chains / fokl_resample_report
 *                              many independent Gibbs chains of a fitted model, drawing their own counter-based numbers
 *                              (fokl_gpy_amd/resample.py)
 *   fokl_robust_pass / fokl_robust_step / fokl_robust_chains / fokl_robust_report / fokl_robust_rng
 *                              Gibbs chains under Student-t noise and given row weights: a weighted pass over the rows per
 *                              iteration (fokl_gpy_amd/robust.py), one pass or one step alone, what the last call ran, and
 *                              the host's view of their random numbers
 *   fokl_score_rows / fokl_score_rows_noise / fokl_score_report
 *                              the log predictive density of every row over all draws: WAIC and PSIS-LOO
 *                              (fokl_gpy_amd/score.py), and what its last launch ran
 *   fokl_predictive_rows / fokl_predictive_rows_noise / fokl_predictive_report
 *                              the predictive distribution of every row over all draws: PIT, quantiles and their brackets
 *                              (fokl_gpy_amd/predictive.py), and what its last launch ran
 *   fokl_design_select / fokl_design_report
 *                              greedy D- / I-optimal selection from a candidate pool (fokl_gpy_amd/design.py), and what
 *                              its last call ran
 *   fokl_acquire_select / fokl_acquire_report
 *                              expected improvement and probability of improvement over a candidate pool, greedy batch
 *                              selection with lazy evaluation (fokl_gpy_amd/acquire.py), and what its last call ran
 *   fokl_acquire_system_select / fokl_acquire_system_incumbent / fokl_acquire_system_report
 *                              the same selection under limits on other models' outputs, feasibility per (row, draw); the
 *                              best objective over the feasible measured rows per draw; what the last of either ran
 *   fokl_drawbest_rows / fokl_drawbest_report
 *                              for every posterior draw its best rows of a candidate pool, ranked
 *                              (fokl_gpy_amd/pooloptimum.py), and what its last call ran
 *   fokl_infer_inputs / fokl_infer_report / fokl_infer_rng
 *                              unknown inputs inferred from observed outputs: one affine-invariant ensemble of 64 walkers
 *                              per posterior draw (fokl_gpy_amd/infer.py), what its last launches ran, and its
 *                              counter-based random numbers as the host sees them
 *   fokl_gp_integrate_report   what the last fokl_gp_integrate_ensemble (fokl_hip.h) ran: the kernel instance, its LDS, the
 *                              band kernel's list and grid
 *   fokl_simulate_ensemble / fokl_simulate_report
 *   fokl_simulate_adaptive / fokl_simulate_adaptive_report
 *   fokl_simulate_stiff / fokl_simulate_stiff_report
 *   fokl_steady_states / fokl_steady_report
 *   fokl_assimilate_ensemble / fokl_assimilate_report / fokl_assimilate_rng
 *   fokl_calibrate_ensemble / fokl_calibrate_report / fokl_calibrate_rng
 *   fokl_control_solve / fokl_control_report
 *   fokl_control_pooled_solve / fokl_control_pooled_report
 *   fokl_control_cvar_solve / fokl_control_cvar_report
 *                              a system of fitted models, wired by names, integrated for every posterior draw at once
 *                              (fokl_gpy_amd/dynamics.py), and what its last call ran
 *   fokl_embedded_hmc / fokl_embedded_rng
 *                              the HMC chains of GPs embedded in a user equation (fokl_gpy_amd/embedded.py) and their
 *                              counter-based random numbers as the host sees them
 *
 * Same conventions as fokl_hip.h (return codes, row-major fp64, FR = /root/reference/src/FoKL/FoKLRoutines.py).
 */
#ifndef FOKL_HIP_INTERNAL_H
#define FOKL_HIP_INTERNAL_H

#include <stddef.h>

#include "fokl_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------------ */
/* The random stream in two phases: bulk threads + one serial walk (round 4; csrc/fokl_stream.cpp).          */
/* Call sites replaced: np.random.normal FR:1527, np.random.gamma FR:1541 / FR:1547.                         */
/* ------------------------------------------------------------------------------------------------------ */

/*
 * The stream of fokl_noise_tape, produced by `bulk_threads` threads ahead of ONE walking thread.  The bulk threads
 * continue MT19937 from the state handed to fokl_stream_create (np.random.get_state()), temper the words and flag, for
 * every double of the stream, whether the polar attempt that STARTS there is accepted (both pairings of the doubles: a
 * gamma's uniform shifts the pairing by one).  fokl_stream_walk advances over one model evaluation's draws exactly
 * as fokl_noise_tape does -- same positions, same consumption, same cached value -- but touches only what is serial: per
 * Gibbs iteration it steps over ceil((p1 - lead) / 2) accepted attempts by counting flags and makes the two gamma draws
 * -- and those from BOUNDS where they decide (a normal is known by its source, the accepted attempt it comes from and
 * which half; its value is formed, with libm's log, only when a gamma's accept test is too close to call: 1 in 10).  A
 * tape row is 32 bytes of positions:
 *     start        double index where the iteration's attempts begin; bit 63 = the row opens with the cached normal
 *     lead_source  the attempt whose x1 half that cached normal is
 *     gamma[2]     source of the normal X the accepted attempt of each gamma draw used (bit 63 = the x1 half): the
 *                  variate is b (1 + c X)^3; all ones = the walker stored the variate itself (shapes <= 1)
 * fokl_stream_expand turns rows back into fokl_noise_tape's layout (raw pairs (x2, x1), r2, lead, final lead / tail
 * values, the two gamma variates) on any thread -- values identical to fokl_noise_tape's; the part of the stream a tape
 * covers must be HELD from before its walk until its last expansion: fokl_stream_hold (on the walking thread, at the
 * position the tape starts from) / fokl_stream_release (any thread).  The walker itself keeps everything from its floor
 * on; fokl_stream_advance_floor moves the floor to its present position (between tapes).
 * fokl_stream_tell / fokl_stream_seek save and restore the walker (tentative tapes: a rewind is three words, the
 * bulk data does not move).  fokl_stream_state writes numpy's state tuple at the walker's position.
 * One thread at a time may walk / seek / tell / ask for the state; expand, hold-release and stats are thread-safe.
 */
#define FOKL_SEGMENT_BLOCKS 256                      /* MT19937 blocks per segment of the stream */
#define FOKL_SEGMENT_DOUBLES 79872                  /* = 256 * 624 / 2 doubles per segment */
#define FOKL_ROW_LEAD (1ull << 63)                  /* fokl_tape_row.start: the row opens with the cached normal */
#define FOKL_SOURCE_X1_HALF (1ull << 63)            /* a normal's source: the x1 half of the attempt (else x2) */
#define FOKL_SOURCE_GIVEN ((1ull << 62) - 1)        /* source position: the cached normal of the state handed over */
#define FOKL_GAMMA_FINAL_VALUE (~0ull)              /* fokl_tape_row.gamma[j]: the walker stored the variate itself */
#define FOKL_PRESTATE_WORDS 640                     /* one entry of the pre-state ring (see fokl_stream_create) */
#define FOKL_PRESTATE_BLOCKS 32                     /* a pre-state is left every 32 blocks: 8 per segment */
typedef struct fokl_stream fokl_stream;
typedef struct fokl_tape_row {
    uint64_t start;
    uint64_t lead_source;
    uint64_t gamma[2];
} fokl_tape_row;
typedef struct fokl_stream_cursor {
    uint64_t position;
    uint64_t gauss_source;
    int32_t has_gauss;
} fokl_stream_cursor;
/* prestate_ring (may be NULL) [prestate_entries * FOKL_PRESTATE_WORDS]: for a second consumer that regenerates the stream
 * itself (the device: fokl_dchain_*), the bulk threads leave there, for every run of FOKL_PRESTATE_BLOCKS blocks and in
 * order, entry index % prestate_entries (index = segment * 8 + run) = the 624 raw words of the MT19937 block in front of
 * the run (the very first: block 0 itself, word 626 = 1), the index (words 624, 625) and the word parity the doubles pair
 * up from (word 627); fokl_stream_prestates_published counts the SEGMENTS whose eight entries are there. */
int fokl_stream_create(const uint32_t *mt_key, int32_t mt_pos, int32_t has_gauss, double gauss_cache, int bulk_threads,
                       uint32_t *prestate_ring, int prestate_entries, fokl_stream **out);
int64_t fokl_stream_prestates_published(const fokl_stream *stream);
double fokl_stream_given_gauss(const fokl_stream *stream);
void fokl_stream_destroy(fokl_stream *stream);
int fokl_stream_walk(fokl_stream *stream, int p1, int draws, double astar, double atau_star, fokl_tape_row *rows,
                     double *gam_sig, double *gam_tau, int32_t *progress);
int fokl_stream_tell(const fokl_stream *stream, fokl_stream_cursor *out);
int fokl_stream_seek(fokl_stream *stream, const fokl_stream_cursor *at);
int fokl_stream_hold(fokl_stream *stream, uint64_t *position_out);
int fokl_stream_release(fokl_stream *stream, uint64_t position);
int fokl_stream_advance_floor(fokl_stream *stream);
int fokl_stream_state(fokl_stream *stream, uint32_t *key_out, int32_t *pos_out, int32_t *has_gauss_out,
                      double *gauss_out);
int fokl_stream_expand(fokl_stream *stream, int p1, double astar, double atau_star, const fokl_tape_row *rows, int k0,
                       int k1, double *normals_out, double *pair_r2_out, int32_t *lead_out, double *gam_sig_out,
                       double *gam_tau_out);
/* seconds the bulk threads worked, seconds the walker waited for them, segments (79 872 doubles each) produced, gamma
 * attempts walked and how many of them needed the exact expressions */
/* Helper threads for the walk: the walking thread then only counts accepted attempts (the chase) and hands blocks of 128
 * iterations out; helpers turn ranks into positions / rows and run the gamma draws' accept tests.  count 0: none (default),
 * at most 4; cpus (may be NULL): the logical CPU of each helper (< 0: not pinned).  Call before the first walk. */
int fokl_stream_set_helpers(fokl_stream *stream, int count, const int32_t *cpus);
/* bulk thread i runs on logical CPU cpus[i % count] only (csrc/fokl_stream.cpp) */
int fokl_stream_place_bulk(fokl_stream *stream, const int32_t *cpus, int count);
int fokl_stream_stats(const fokl_stream *stream, double *bulk_busy_s, double *walker_wait_s, int64_t *segments,
                      int64_t *gamma_attempts, int64_t *gamma_attempts_exact);
/* max |fast_ln(y) - log(y)| over a sweep of (0, 1): the approximation the walker's bounds are built on (tests) */
double fokl_stream_fast_ln_error(int64_t n);

/* ------------------------------------------------------------------------------------------------------ */
/* Host threads of one fit: the work of G2/G3 that must not sit on the Python driver thread.                */
/* ------------------------------------------------------------------------------------------------------ */

typedef struct fokl_host_pool fokl_host_pool;
typedef struct fokl_host_job fokl_host_job;

/*
 * One noise thread that walks the random stream (fokl_stream_*: created here from mt_key / mt_pos / has_gauss / gauss_cache
 * -- caller storage, read now and WRITTEN BACK by fokl_pool_destroy with numpy's state after everything that was walked --
 * and produced by `bulk_threads` threads of its own) and records tapes strictly in submission order, `finish_threads`
 * threads that materialise each tape (all of them on every tape; 0 = the noise thread does it, block by block),
 * `chain_threads` threads that run the chain recursions and `spectral_threads` threads that diagonalise XtX sub-blocks.
 * `dsyevr` is the address of LAPACK's dsyevr with the Fortran calling convention and 32-bit integers (the Python side
 * passes scipy's own: scipy.linalg.cython_lapack.__pyx_capi__['dsyevr']), so that eigenpairs are those of the reference's
 * scipy.linalg.eigh call (FR:1499) bit for bit; NULL is allowed with spectral_threads == 0.
 * The threads inherit the CPU affinity of the caller, except that the noise thread is pinned to logical CPU
 * `noise_cpu` if that is >= 0 (the caller then keeps its other threads off that core).  Every buffer handed to a submit
 * call must stay alive until fokl_pool_wait has returned for that job.  fokl_pool_destroy first runs everything still queued.
 */
int fokl_pool_create(int chain_threads, int finish_threads, int spectral_threads, int bulk_threads, int noise_cpu,
                     void *dsyevr, uint32_t *mt_key, int32_t *mt_pos, int32_t *has_gauss, double *gauss_cache,
                     uint32_t *prestate_ring, int prestate_entries, fokl_host_pool **out);
/* Models of from_columns columns or more are diagonalised by LAPACK's divide-and-conquer driver dsyevd (fn: its address,
 * Fortran ABI with 32-bit integers, e.g. scipy.linalg.cython_lapack's) instead of dsyevr: the same tridiagonal reduction,
 * eigenpairs within ~3e-12 of dsyevr's in the chain's noise map, 1.3-1.5 x faster from 80 columns on, 2 x at 585.  NULL or
 * 0: dsyevr (what scipy.linalg.eigh calls, FR:1499) for every size.  Call before the first spectral job. */
int fokl_pool_use_dsyevd(fokl_host_pool *pool, void *fn, int from_columns);
/* BLAS dgemm (fn: its address, Fortran ABI with 32-bit integers, e.g. scipy.linalg.cython_blas's) for the product of
 * fokl_pool_submit_spectral_update; NULL: those jobs decompose afresh.  Call before the first spectral job. */
int fokl_pool_use_dgemm(fokl_host_pool *pool, void *fn);
/* The same product on the device (csrc/fokl_dgemm_device.inc): fokl_device_dgemm has BLAS dgemm's signature and runs
 * C = A B ('N', 'N', alpha 1, beta 0; N and K of at least `from`, M of at least 16) as fp64 MFMA tiles on `device` through
 * page-locked staging buffers of the calling thread; every other call, and any device failure, goes to host_dgemm.
 * fokl_device_dgemm_configure returns its address through *entry -- what to give fokl_pool_use_dgemm for searches whose
 * models have hundreds of columns (585: 0.4 GFLOP per derived model, 8-10 ms on a host core).  One configuration per
 * process.  Replaces the call of scipy's dgemm inside the eigen-update (no reference line: the reference decomposes every
 * model afresh, FR:1499). */
void fokl_device_dgemm(char *transa, char *transb, int *m, int *n, int *k, double *alpha, double *a, int *lda, double *b,
                       int *ldb, double *beta, double *c, int *ldc);
int fokl_device_dgemm_configure(int device, void *host_dgemm, int from, void **entry);
int fokl_device_dgemm_stats(int64_t *calls, int64_t *on_device, int64_t *failed);

/* CPUs for the spectral threads alone (they share no data with the threads around the random stream: another last-level
 * cache domain keeps them off those threads' cores) */
int fokl_pool_spectral_affinity(fokl_host_pool *pool, const int32_t *cpus, int count);
/* the pool's stream (fokl_stream_expand of rows-only tapes; alive as long as the pool) */
fokl_stream *fokl_pool_stream(fokl_host_pool *pool);
void fokl_pool_destroy(fokl_host_pool *pool);
/* 1 = every row of the tape is recorded (progress == draws) and every block of `block` rows is there (block_done[] != 0:
 * expanded / finished by the pool's finish threads), 0 = not yet, -1 = it never will be.  Acquire loads: a consumer on any
 * thread may poll this before it reads the tape's arrays.  Either pointer may be NULL (not looked at). */
int fokl_tape_ready(const int32_t *progress, int draws, const int32_t *block_done, int block);

/*
 * One model evaluation's tape on the noise thread: fokl_stream_walk into rows [draws] (progress must be given and start
 * at 0: rows walked so far), materialised into fokl_noise_tape's layout (normals / pair_r2 / lead / gam_sig / gam_tau:
 * identical numbers) by the finish threads, block by block of `block` rows behind the walk: block_done [ceil(draws /
 * block)] (zero-initialised) receives 1 (release) per block, -1 if the tape is sent back.  finish != 0: the normals of
 * each block are also completed IN PLACE (the log / sqrt half of the polar method: tapes a host chain reads); the job
 * counts as run only when the finish threads have left the tape too.  finish == 2: ROWS ONLY -- nobody materialises
 * the tape here (normals / pair_r2 / lead / block_done may be NULL): a consumer that has the stream itself expands the
 * rows (the device: fokl_dchain_submit_rows; or fokl_stream_expand on fokl_pool_stream).
 * span_out (may be NULL; required with finish == 2) receives [position the stream is held from for this tape, walker
 * position behind the tape] before progress reaches `draws`; the hold is then the CALLER's: fokl_pool_release_hold
 * when nobody will expand the rows any more.
 * tentative != 0: the tape is walked ahead of the decision that it is needed, and fokl_pool_resolve(job, commit) is
 * its verdict -- commit keeps the tape (identical to a plain submission at that point of the stream), otherwise the
 * walker is put back where the tape began and `progress` is set to -1.  Tentative tapes may be NESTED: up to 16 can be
 * on record without a verdict, the noise thread goes on walking behind them.  A commit of the oldest makes it final;
 * an abort takes every younger tentative tape with it (the caller resolves those to "abort" as well: what they hold is
 * no longer what the stream serves there); an abort of the youngest rewinds just that one.  A plain request waits until
 * nothing tentative is left.  Every tentative job MUST be resolved, or the noise thread (and fokl_pool_destroy) waits
 * for ever.
 */
int fokl_pool_submit_noise(fokl_host_pool *pool, int p1, int draws, double astar, double atau_star, fokl_tape_row *rows,
                           double *normals, double *pair_r2, int32_t *lead, double *gam_sig, double *gam_tau,
                           int32_t *progress, int tentative, int32_t *block_done, int block, int finish,
                           uint64_t *span_out, fokl_host_job **out);
int fokl_pool_release_hold(fokl_host_pool *pool, uint64_t position);
int fokl_pool_resolve(fokl_host_job *job, int commit);
/*
 * The draws of one candidate from its tape (whose noise job must have been submitted with the same block_done): the
 * recursion follows the flags of the finish threads -- on normals they completed in place (finishing_requested != 0:
 * the tape was submitted with finish != 0) or completing each row itself.  then (may be NULL): called with then_arg by the
 * chain thread once the chain has run without error, before the job counts as done (what follows from the complete draws).
 */
int fokl_pool_submit_chain(fokl_host_pool *pool, const double *lamb, const double *qty, int p1, double b, double btau,
                           double dtd, double sigsqd0, double tausqd0, int draws, const double *normals,
                           const double *pair_r2, const int32_t *lead, const double *gam_sig, const double *gam_tau,
                           const int32_t *progress, int32_t *block_done, int block, int finishing_requested,
                           double *w_out, int32_t *bstar_negative, void (*then)(void *), void *then_arg, fokl_host_job **out);
/*
 * G2 for the candidate model made of columns idx[0..p1) of `gram` (row-major, leading dimension ld, y in column
 * ycol): XtX = gram[idx][:, idx], Xty = gram[idx, ycol].  Outputs: lamb_out [p1] ascending eigenvalues,
 * qt_out [p1, p1] with ROW j = eigenvector j (largest-magnitude component positive), qty_out = Q'Xty,
 * betahat_out = Q (qty / lamb) (FR:1499-1504).  moments_out [2] (may be NULL) receives sum r and sum r^2 of the
 * residual r = y - X betahat, formed from the Gram alone -- sum y - 1'X b and y'y - 2 b'Xty + b'XtX b in extended
 * precision; column 0 of gram must be the ones column -- the quantities fokl_bic_resid measures on the device
 * (FR:1551).  No random numbers: may be submitted speculatively.
 */
int fokl_pool_submit_spectral(fokl_host_pool *pool, const double *gram, int ld, const int32_t *idx, int p1, int ycol,
                              double *lamb_out, double *qt_out, double *qty_out, double *betahat_out,
                              double *moments_out, fokl_host_job **out);
/* G2 of a kill test's model (FR:1666-1690 evaluate the current model minus one term) from the eigenpairs of the model with
 * that ONE MORE column instead of from scratch: parent_lamb [p1 + 1] ascending, parent_qt [p1 + 1, p1 + 1] as qt_out above,
 * parent_pos = which of the parent's columns this model lacks.  The eigenvalues are the roots of the secular equation
 * sum_j z_j^2 / (lam_j - mu) = 0 (z = row parent_pos of Q), the eigenvectors one (p1 x (p1+1) x p1) dgemm; vectors from the
 * z^ of Gu & Eisenstat, so orthogonal to working precision.  parent_job: NULL when the parent's arrays are complete, else
 * the spectral job of this pool that writes them (not waited for yet): this job is queued, ahead of everything else, when
 * that one has run.  updated (may be NULL): 1 = derived from the parent, 0 = decomposed afresh after all (the parent
 * failed, nearly repeated eigenvalues or vanishing z_j -- no deflation here --, a failed check of diag(XtX) against the
 * eigenpairs, no dgemm bound, FOKL_EIGH_SIGNS=lapack).  Same outputs, layout and sign convention as
 * fokl_pool_submit_spectral; accuracy: tests/stress/eigen_deletion_study.py. */
int fokl_pool_submit_spectral_update(fokl_host_pool *pool, const double *gram, int ld, const int32_t *idx, int p1, int ycol,
                                     const double *parent_lamb, const double *parent_qt, int parent_pos,
                                     fokl_host_job *parent_job, double *lamb_out, double *qt_out, double *qty_out,
                                     double *betahat_out, double *moments_out, int32_t *updated, fokl_host_job **out);
/* 1 if the job has run.  fokl_pool_wait blocks until then, frees the job and returns its status. */
int fokl_pool_poll(const fokl_host_job *job);
int fokl_pool_wait(fokl_host_job *job);
/* Accumulated time (s) the kinds of thread spent inside jobs (including their waits on the tape producer). */
int fokl_pool_busy_seconds(const fokl_host_pool *pool, double *noise, double *chain, double *finish,
                           double *spectral);
/* The pool's random stream: fokl_stream_stats of it. */
int fokl_pool_stream_stats(const fokl_host_pool *pool, double *bulk_busy_s, double *walker_wait_s, int64_t *segments,
                           int64_t *gamma_attempts, int64_t *gamma_attempts_exact);
/* Seconds the noise thread spent waiting: with an empty queue, and for the verdict on tentative tapes. */
int fokl_pool_noise_waits(const fokl_host_pool *pool, double *queue_wait, double *verdict_wait);
/* CPU-seconds the library's own threads have used since it was loaded, by kind, process-wide (a pool's threads are added
 * when they end, i.e. when their fit's pool is destroyed): seconds[0..5] = the stream's walker, chain threads, finish
 * threads, spectral threads, the stream's bulk threads, the device-chain dispatchers (live).  -> 6, or an error.  What a fit
 * costs in CPU and where: the figure that bounds fits running side by side on a host with a CPU quota. */
int fokl_thread_cpu_seconds(double *seconds, int count);

/* ------------------------------------------------------------------------------------------------------ */
/* A host chain's recursion in verified segments (csrc/fokl_sampler.cpp, csrc/fokl_chain_lanes.inc)          */
/* ------------------------------------------------------------------------------------------------------ */

/* How a chain is cut, on the device (gibbs_chain_segments_kernel) and on the host: pieces, and the iterations a piece
 * starts early. */
#define FOKL_CHAIN_SEGMENTS 8
#define FOKL_CHAIN_WARM 64

/*
 * fokl_gibbs_chain_from_finished_tape (same arguments, same waiting on block_done) with the draws cut into `segments`
 * pieces (1..8) when draws >= 4 * warm, one piece otherwise: piece s runs iterations [max(s piece - warm, 0),
 * min((s + 1) piece, draws)), piece = ceil(draws / segments), from (sigsqd0, tausqd0) and writes nothing before s piece.
 * Accepted if every non-empty piece but the first holds, in front of its first own iteration, the state the piece before
 * it ended on (both scalars, |have - want| <= 1e-14 |want|) and no piece met bstar < 0; otherwise the one-piece function
 * runs from the initial state, every row is rewritten and *bad_cut = 1 (NULL allowed) -- a flagged chain returns exactly
 * what fokl_gibbs_chain_from_finished_tape returns.  Within a piece an iteration is the one-piece function's, bit for bit
 * from the same entering state, in the portable, AVX2 and AVX-512 statements alike (FOKL_CHAIN_ISA).  The pieces run in
 * the SIMD lanes of the calling thread; FOKL_HCHAIN_MAPPING=pieces runs them one after the other (tests), and
 * FOKL_HCHAIN_RECURSION=serial calls the one-piece function whatever the arguments.
 */
int fokl_gibbs_chain_segments_host(const double *lamb, const double *qty, int p1, double b, double btau, double dtd,
                                   double sigsqd0, double tausqd0, int draws, const double *normals,
                                   const double *gam_sig, const double *gam_tau, const int32_t *block_done, int block,
                                   double *w_out, double *sigs_out, double *taus_out, int32_t *bstar_negative,
                                   int segments, int warm, int32_t *bad_cut);
/* Host chains of this pool that ran in segments, and those among them that failed the check and ran again in one piece. */
int fokl_pool_chain_segments(const fokl_host_pool *pool, int64_t *segmented, int64_t *recuts);

/* ------------------------------------------------------------------------------------------------------ */
/* The search's per-evaluation work off the driver thread: tapes on order, G2 ahead, chains, kill tests     */
/* (csrc/fokl_search.cpp).  Replaces the loop FR:1666-1690 and the bookkeeping around FR:1650 / FR:1681.     */
/* ------------------------------------------------------------------------------------------------------ */

/*
 * A fokl_search holds, for ONE fit, what the sequential decisions of the forward selection share: the queue of noise
 * tapes on order ahead of the decisions that they are needed, the G2 jobs submitted ahead, the chains (pool threads or
 * the device engine), the decisions taken from guessed intercept scales and their confirmation, the BIC cache of models
 * scored before, the trace of evaluations.  It is driven by one thread.  The driver (Python: engine.ForwardSelection)
 * keeps the sequence of sub-stages, the K1 / K2 / K3 launches, the statistics that order a sub-stage's proposals and the
 * stop rule, and calls
 *   fokl_search_set_substage        term ids of the active columns (identical models score identically, see
 *                                   fokl_search_score);
 *   fokl_search_model_begin/_commit a sub-stage's model (FR:1650) around the driver's residual pass;
 *   fokl_search_score               BIC (FR:1551-1554, 1653-1654) from residual moments + the trace record;
 *   fokl_search_kill_tests          FR:1666-1690 for one sub-stage: same tests, same order, same consumption of the
 *                                   random stream; BIC of the candidates from the sub-stage's Gram.
 * dchain may be NULL (every chain on pool threads).  fokl_search_destroy sends back what is on order and waits for
 * everything in flight; the pool must outlive the search.
 */
typedef struct fokl_dchain fokl_dchain;         /* the device chain engine, declared further down */
typedef struct fokl_search fokl_search;
typedef struct fokl_spectrum fokl_spectrum;     /* one G2 job and its result */
typedef struct fokl_tape fokl_tape;             /* one model evaluation's noise */
typedef struct fokl_outcome fokl_outcome;       /* one model evaluation */
typedef struct fokl_search_params {
    int64_t n;                                  /* rows of the whole dataset (FR:1508: astar) */
    double a, b, atau, btau;                    /* FR:1322-1348 */
    double threshav, threshstda, threshstdb;    /* FR:1670-1671 */
    double guess_margin;                        /* decisions from the least-squares intercept: relative distance kept */
    int32_t draws;                              /* burnin + draws: iterations per chain */
    int32_t half0;                              /* ceil(draws / 2): first row of the intercept statistic (FR:1671) */
    int32_t aic;                                /* FR:1653-1654 */
    int32_t lookahead, foresight;               /* G2 jobs ahead of the tests; tests left when the next model is foreseen */
    int32_t speculation_max;                    /* tapes on order at most */
    int32_t tentative_tapes, test_rewinds;      /* 0: no tape is ordered ahead; tests: a discarded tape before every order */
    int32_t device_chain_columns;               /* device chains for models of up to this many columns */
    int32_t finish_threads;                     /* of the pool (0: chains complete their normals themselves) */
    int32_t flip_guess;                         /* tests: the n-th guessed decision is taken wrong */
    int32_t device_rows;                        /* the pool's stream leaves its pre-states with dchain: kill tests' tapes
                                                   stay rows, the device expands them (fokl_dchain_submit_rows) */
} fokl_search_params;
int fokl_search_create(fokl_host_pool *pool, fokl_dchain *dchain, const fokl_search_params *params, fokl_search **out);
/* G2 on the device engine (fokl_dspectral_*, declared further down; NULL: everything back to the pool's LAPACK threads)
 * for models of up to max_columns columns whose result is not wanted before the device can have it: a job requested
 * `slack` times the kernels' duration (or more) ahead of its kill test goes to the device, the others to the pool;
 * slack = 0: all of them, < 0: the default (1.5).  lookahead: how many tests ahead device jobs are requested (< 0: the
 * default, 32; the pool's jobs stay at fokl_search_params.lookahead).  Between fokl_search_hold_spectral(s, 1) and (s, 0)
 * fokl_search_spectral only stages its jobs; the closing call launches them as one grid. */
typedef struct fokl_dspectral fokl_dspectral;
int fokl_search_bind_spectral(fokl_search *search, fokl_dspectral *engine, int max_columns, double slack, int lookahead);
int fokl_search_hold_spectral(fokl_search *search, int hold);
/* G2 of the kill tests' models from the eigenpairs of the model each is tested against (fokl_pool_submit_spectral_update:
 * secular equation + one product, 4-5 x cheaper than a decomposition): for parents of from_columns columns or more (0, the
 * default: never) and at most `depth` such steps away from a fresh decomposition -- a step runs when the one before it has,
 * so `depth` cuts the chain of accepted tests along the predicted path into pieces the spectral threads work on side by side.
 * A chain of derivations advances slower than the loop tests and only the pieces inside the look-ahead window run side by
 * side: `lookahead` (0: fokl_search_params.lookahead) is the window's depth while derivation is on, in sub-stages whose model
 * has fewer than 192 columns.  Statistic 'spectral_updated' counts the models that were derived this way. */
int fokl_search_set_update(fokl_search *search, int from_columns, int depth, int lookahead);
/* How a kill test's BIC (FR:1686: `evtest < evmin`) is decided.  mode 0: from G2 of the trial model -- the loop waits for the
 * eigenpairs of every model it tests (round 4).  mode 1: from the sub-stage model's least-squares fit with the tested columns
 * removed one by one (sum of squared residuals without column c = SSR + b_c^2 / [(X'X)^-1]_cc, (X'X)^-1 and b one rank-one
 * downdate per accepted test): microseconds per test on the search thread; G2 is then requested for ACCEPTED models only,
 * feeds nothing but their chains (started when it arrives) and brings a second BIC (Gram identity on the eigenpairs'
 * betahat) that must agree with the decision's to `tolerance` (relative; <= 0: 1e-9) -- else the search ends as after a
 * mispredicted guess (fokl_search_mispredicted) and the driver repeats it in mode 0.  Sub-stages whose model is
 * numerically singular (smallest eigenvalue <= 1e-9 of the largest) run in mode 0 whatever is set here.  Statistics
 * 'direct_tests', 'direct_max_rel' (largest relative difference seen), 'chains_cancelled' (accepted models replaced
 * before anything looked at their draws: their chains never run). */
int fokl_search_set_decide(fokl_search *search, int mode, double tolerance);
/* Several ranks repeat this search side by side (rows or candidates sharded over GPUs) and must take every decision alike:
 * on != 0 keeps the arrival time of a chain's statistics out of every decision -- a second clause of FR:1670 that can be
 * guessed from the least-squares intercept IS guessed (a function of the all-reduced / all-gathered Gram alone), and a guess
 * that its chain does not confirm ends the search in the blocking fokl_search_verify at its end, where every rank finds it. */
int fokl_search_set_deterministic(fokl_search *search, int on);
void fokl_search_destroy(fokl_search *search);
const char *fokl_search_error(const fokl_search *search);
/* 1 after a guessed decision was not confirmed by its chain (the driver repeats the search without device chains) */
int fokl_search_mispredicted(const fokl_search *search);
int fokl_search_set_substage(fokl_search *search, const int64_t *term_ids, int columns);
/* the models the stream will probably serve next, in order (sizes in columns; is_model: a sub-stage's model) */
int fokl_search_speculate(fokl_search *search, const int32_t *sizes, const int32_t *is_model, int count);
int fokl_search_drop_speculation(fokl_search *search);
/* G2 (fokl_pool_submit_spectral) with the result buffer owned by the search: lamb [p1] | qty [p1] | betahat [p1] |
 * Qt [p1, p1] | moments [2]; gram must stay alive until the job has run */
int fokl_search_spectral(fokl_search *search, const double *gram, int ld, const int32_t *idx, int p1, fokl_spectrum **out);
/* The same for the model that is `parent`'s (a spectrum of this search, waited for or not) without its column number
 * parent_pos (NULL / -1: as fokl_search_spectral): derived from the parent's eigenpairs where fokl_search_set_update allows. */
int fokl_search_spectral_from(fokl_search *search, const double *gram, int ld, const int32_t *idx, int p1,
                              fokl_spectrum *parent, int parent_pos, fokl_spectrum **out);
int fokl_spectrum_done(fokl_spectrum *spectrum);
int fokl_spectrum_wait(fokl_search *search, fokl_spectrum *spectrum, const double **buffer, int *p1);
int fokl_spectrum_retain(fokl_search *search, fokl_spectrum *spectrum);     /* one more reference (released as below) */
void fokl_spectrum_release(fokl_search *search, fokl_spectrum *spectrum);
int fokl_search_model_begin(fokl_search *search, const double *gram, int ld, const int32_t *idx, int p1,
                            fokl_spectrum *given, const int32_t *then_sizes, const int32_t *then_model, int then_count,
                            fokl_spectrum **spectrum_out, fokl_tape **tape_out);
/* model_begin without its wait for G2 (the caller launches what it has, then fokl_spectrum_wait); _abandon gives both
 * references back when the model is not committed after all (a commit, failed or not, has taken them over) */
int fokl_search_model_request(fokl_search *search, const double *gram, int ld, const int32_t *idx, int p1,
                              fokl_spectrum *given, const int32_t *then_sizes, const int32_t *then_model, int then_count,
                              fokl_spectrum **spectrum_out, fokl_tape **tape_out);
void fokl_search_model_abandon(fokl_search *search, fokl_spectrum *spectrum, fokl_tape *tape);
int fokl_search_model_commit(fokl_search *search, fokl_spectrum *spectrum, fokl_tape *tape, double dtd, int new_terms,
                             fokl_outcome **out);
int fokl_search_score(fokl_search *search, fokl_outcome *outcome, double sum_r, double sum_r2, int n_prev, int kill,
                      double *ev);
typedef struct fokl_outcome_view {
    const double *spectrum;                     /* lamb | qty | betahat | Qt | moments of the model */
    const int32_t *idx;                         /* its active-column indices [p1] */
    double ev, siglik, intercept_scale;         /* intercept_scale: NaN while unknown */
    int32_t p1, on_device;
} fokl_outcome_view;
int fokl_outcome_info(fokl_search *search, fokl_outcome *outcome, fokl_outcome_view *view);
int fokl_outcome_spectrum(fokl_search *search, fokl_outcome *outcome, fokl_spectrum **out);
int fokl_outcome_chain_ready(fokl_outcome *outcome);
int fokl_outcome_draws(fokl_search *search, fokl_outcome *outcome, const double **w);
int fokl_outcome_intercept_scale(fokl_search *search, fokl_outcome *outcome, double *scale);
/* FR:1656-1658 for the active columns `cols` of the outcome's model, from its draws in the eigenbasis (waits for the chain):
 * mean_abs[c] = |mean over rows half1 .. of beta_c|, rel_std[c] = std over rows half1 .. / |mean over rows half0 ..|. */
int fokl_outcome_new_term_stats(fokl_search *search, fokl_outcome *outcome, const int32_t *cols, int count, int half0,
                                int half1, double *mean_abs, double *rel_std);
void fokl_outcome_release(fokl_search *search, fokl_outcome *outcome);
void fokl_outcome_drop(fokl_search *search, fokl_outcome *outcome);
int fokl_search_verify(fokl_search *search, int block);
int fokl_search_register_forecast(fokl_search *search, const int32_t *key, int key_count, fokl_spectrum *spectrum,
                                  double dtd);
void fokl_search_clear_forecasts(fokl_search *search);
int fokl_search_likely_first_tests(fokl_search *search, fokl_spectrum *spectrum, int n_new, double siglik,
                                   int32_t *columns_out, int32_t *accepted_out, int *count);
/* counters / seconds in the order of csrc/fokl_search.cpp's Stat enumeration (-> their number); the trace: 5 doubles per
 * evaluation (columns, built, ev, kill, the mean intercept draw over rows half0 .. of that evaluation's chain -- FR:1671's
 * scale before the abs() -- or NaN where the search never looked at that chain's statistics) */
int fokl_search_stats(const fokl_search *search, double *values, int count);
int64_t fokl_search_trace(const fokl_search *search, double *records, int64_t capacity);
/*
 * One sub-stage's kill tests.  gram [(active + 1)^2]: Gram of the active columns with y last; columns / mean_abs /
 * rel_std [proposals]: the new terms in testing order (ascending |mean beta|, FR:1663-1664): active-column index,
 * |mean beta| (FR:1656), std / |mean| (FR:1657-1658); slots [active]: device slot of every active column (the key of
 * forecasts); best: the sub-stage's model.  ahead_*: G2 jobs the caller submitted for first trial sets (keys: active
 * column indices, CSR offsets).  vm_next: columns the coming sub-stage adds (-1: there is none).  Callbacks (may be
 * NULL) run on the calling thread: foresee(predicted kill set) towards the end of the loop; idle_work once, when the
 * first test's tape and G2 are under way (or at the end); residual: sum r, sum r^2 of y - X betahat for a candidate
 * that (nearly) interpolates the data.  killed [>= proposals] receives the kill set (ascending); best: the model the
 * sub-stage ends on (best_is_new: a new handle the caller owns, else the one passed in).
 */
typedef struct fokl_kill_tests_args {
    const double *gram;
    const int32_t *columns;
    const double *mean_abs, *rel_std;
    const int32_t *slots;
    fokl_outcome *best;
    const int32_t *ahead_keys, *ahead_offsets;
    fokl_spectrum *const *ahead_spectra;
    void *user;
    void (*foresee)(void *user, const int32_t *killed, int count);
    int (*idle_work)(void *user);
    int (*residual)(void *user, const int32_t *idx, int p1, const double *betahat, double *sum_r, double *sum_r2);
    int32_t active, proposals, n_prev, vm_next, ahead_count;
} fokl_kill_tests_args;
typedef struct fokl_kill_tests_result {
    int32_t *killed;
    fokl_outcome *best;
    double evmin;
    int32_t killed_count, best_is_new;
} fokl_kill_tests_result;
int fokl_search_kill_tests(fokl_search *search, const fokl_kill_tests_args *args, fokl_kill_tests_result *result);

/* ------------------------------------------------------------------------------------------------------ */
/* The sub-stage loop next to the kill-test loop (round 6; csrc/fokl_run.cpp).  Replaces the bookkeeping of    */
/* FR:1602-1748 around the calls above: enumeration, build-ahead, model evaluation, statistics, stop rule.     */
/* ------------------------------------------------------------------------------------------------------ */
/* The device as a table of entry points with the signatures of fokl_hip.h (ctx is handed back as their first
 * argument): the library's own functions on a fokl_ctx, or a checker backend's callbacks (CPU tests). */
typedef struct fokl_backend_ops {
    void *ctx;
    int (*reserve_slots)(void *ctx, int n_slots);
    int (*build_terms)(void *ctx, const int32_t *terms, int T, const int32_t *slots);
    int (*gram)(void *ctx, const int32_t *row_slots, int nr, const int32_t *col_slots, int nc, double *out, int path,
                int allreduce);
    int (*gram_launch)(void *ctx, const int32_t *row_slots, int nr, const int32_t *col_slots, int nc, int allreduce);
    int (*gram_fetch)(void *ctx, double *out, int64_t count);
    int (*gram_ready)(void *ctx);                                       /* may be NULL */
    int (*bic_resid)(void *ctx, const int32_t *slots, int nc, const double *betahat, double *out, int allreduce);
    int (*bic_resid_launch)(void *ctx, const int32_t *slots, int nc, const double *betahat);
    int (*bic_resid_fetch)(void *ctx, double *out, int allreduce);
    int (*bic_resid_terms_launch)(void *ctx, const int32_t *terms, int n_terms, const double *betahat);   /* may be NULL */
    int32_t kernel_id;                                                  /* FOKL_KERNEL_* of the uploaded dataset */
} fokl_backend_ops;
typedef struct fokl_run_params {
    int32_t m, n_phis;                          /* inputs; orders the kernel offers (FR:1747) */
    int32_t way3, tolerance, gimmie;            /* FR:208-212 */
    int32_t draws, half0;                       /* iterations per chain; first row of the intercept statistic */
    int32_t lookahead, lookahead_native, foresight, speculate_across;   /* engine.py's knobs of the same names */
    int32_t forecast_early, forecast_polls;
    int32_t matrix_free;                        /* K3 without the stored columns where the terms allow it */
    int32_t update_from, update_depth, update_lookahead;   /* fokl_search_set_update's arguments (update_depth 0: never set) */
    int32_t head_start;                         /* fokl_run_create launches the first sub-stage's K1 + K2 */
    int32_t slot_capacity;                      /* device column slots to start with */
} fokl_run_params;
#define FOKL_RUN_STATS 16
typedef struct fokl_run fokl_run;
/* Seed Gram + (head_start) the first sub-stage's columns and Gram block under way: before the caller creates its pool. */
int fokl_run_create(const fokl_backend_ops *ops, const fokl_run_params *params, fokl_run **out);
/* fokl_search_set_update's arguments as the caller configured its search (the loop shortens the derivation depth in the
 * sub-stage after which the stop rule may end the search; depth 0: never touched). */
int fokl_run_set_update(fokl_run *run, int from_columns, int depth, int lookahead);
/* The loop, on `search` (fokl_search_create on the caller's pool; decisions, update depth etc. configured by the caller). */
int fokl_run_search(fokl_run *run, fokl_search *search);
/* What it found: rows of the interaction matrix, length of the BIC trace, sub-stages; the outcome handles of the returned
 * model and of the last sub-stage's survivor (the caller owns them: fokl_outcome_drop; they may be one and the same). */
int fokl_run_result(const fokl_run *run, int32_t *mtx_rows, int32_t *evs_count, int32_t *substages,
                    fokl_outcome **best_model, fokl_outcome **last_model);
/* mtx [mtx_rows][m], evs, per sub-stage the number of new terms and -- concatenated -- their |mean beta| and std / |mean|
 * (FR:1656-1658), stats [FOKL_RUN_STATS]: columns built, sub-stages, forecasts used / early, matrix-free residual passes,
 * seconds waiting for K3, seconds by phase (prepare, model, statistics, tests, wrap-up).  NULL: skipped.  -> length of the
 * statistics arrays */
int fokl_run_arrays(const fokl_run *run, int32_t *mtx, double *evs, int32_t *stat_sizes, double *stat_mean_abs,
                    double *stat_rel_std, double *stats);
/* In which order a sub-stage's model went out: per sub-stage FOKL_RUN_ORDER_STAMPS readings of the monotonic clock (seconds)
 * -- K1 of the coming sub-stage launched, wait for G2 begun, G2 arrived, chain submitted, first tests' orders placed, K3
 * launched, the coming sub-stage's Gram launched; NaN: that step did not happen there.  stamps [capacity rows] (NULL: only
 * count) -> sub-stages recorded */
#define FOKL_RUN_ORDER_STAMPS 7
int fokl_run_order(const fokl_run *run, double *stamps, int capacity);
const char *fokl_run_error(const fokl_run *run);
void fokl_run_destroy(fokl_run *run);

/* ------------------------------------------------------------------------------------------------------ */
/* G3 on the device: finishing of the polar normals + the D-iteration recursion (FoKLRoutines.py:1519-1548)  */
/* ------------------------------------------------------------------------------------------------------ */

/* A device-chain engine on HIP device `device`: a dispatcher thread, a few streams, `slots` chains that may be
 * alive (in flight, or finished with their draws still in device memory) at a time.  The random stream stays on
 * the host (fokl_noise_tape / the pool's noise thread); what is submitted here is the arithmetic on a tape:
 * the sqrt(-2 log r2 / r2) half of the polar method and the recursion in the eigenbasis that fokl_gibbs_chain
 * runs on the host -- same operations in the same order, so the draws differ only through log() (1e-16).
 *
 * fokl_dchain_submit queues a chain and returns at once.  The tape may still be on record: `progress` (may be
 * NULL: the tape is complete) is polled by the dispatcher until it reaches `draws`; a negative value fails the
 * job; `block_done` / `block` (may be NULL: the arrays are filled as soon as `progress` says so) are the flags of the
 * threads that materialise the tape (fokl_pool_submit_noise), polled the same way.  `finished` != 0: the normals are
 * final already (host finish threads), else they are raw pairs + `lead` as fokl_noise_tape leaves them.  lamb / qty are copied at submit; the tape's arrays must stay valid until fokl_dchain_poll
 * reports 1 or fokl_dchain_wait / fokl_dchain_release has returned.
 * fokl_dchain_wait sleeps until the chain has run and returns stats_out[4 + p1] = {bstar < 0 seen, last sigma^2,
 * last tau^2, rows averaged, mean over rows stat_first .. draws - 1 of w} -- what the kill tests look at
 * (FR:1671: mean intercept draw = mean w . Q[0, :]).  fokl_dchain_fetch_w copies the draws in the eigenbasis
 * w [draws, p1] (betas = w Q') to the host; fokl_dchain_release frees the slot (idempotent).
 * `stats_area` (may be NULL) receives the address of the job's statistics in page-locked host memory: the seven + p1
 * doubles the recursion kernel writes -- the four + p1 of fokl_dchain_wait, then the job's ticket (as a double),
 * stored last with system-wide release semantics: a caller may poll that word instead of calling fokl_dchain_poll;
 * behind it the seconds the chain's kernel ran (its own clock), and 1.0 when the segmented recursion found that the
 * chain does not forget its state within a warm-up and ran it again in one piece (0.0 otherwise).
 * The area belongs to the job's slot: valid until the job is released.
 * Errors: FOKL_ERR_STATE when every slot is taken (the caller runs that chain on the host). */
int fokl_dchain_create(int device, int slots, fokl_dchain **out);
void fokl_dchain_destroy(fokl_dchain *engine);
int fokl_dchain_submit(fokl_dchain *engine, int p1, int draws, const double *lamb, const double *qty, double b,
                       double btau, double dtd, double sigsqd0, double tausqd0, const double *normals,
                       const int32_t *lead, const double *gam_sig, const double *gam_tau, const int32_t *progress,
                       const int32_t *block_done, int block, int finished, int stat_first, int64_t *ticket,
                       const double **stats_area);
/*
 * The tape as ROWS (round 4): the engine keeps its own copy of the random stream -- fokl_dchain_prestate_ring hands out the
 * page-locked ring a stream created with it (fokl_stream_create / fokl_pool_create) leaves its pre-states in, one
 * workgroup per segment regenerates MT19937 -> tempering -> numpy's doubles -> x = 2 d - 1 from a pre-state into a ring in
 * device memory (when a chain first needs the segment), fokl_dchain_bind_stream says whose pre-states the ring holds -- and
 * fokl_dchain_submit_rows expands a tape's 32-byte rows there: accepted attempts re-decided from x1^2 + x2^2 (the host's
 * roundings: same flags), normals finished, gamma variates formed.  What crosses the bus per chain is its rows; the
 * arithmetic differs from the host's expansion only through log().
 */
int fokl_dchain_prestate_ring(fokl_dchain *engine, uint32_t **ring, int *entries);
int fokl_dchain_bind_stream(fokl_dchain *engine, const fokl_stream *stream);
int fokl_dchain_submit_rows(fokl_dchain *engine, int p1, int draws, const double *lamb, const double *qty, double b,
                            double btau, double dtd, double sigsqd0, double tausqd0, double astar, double atau_star,
                            const fokl_tape_row *rows, const double *gam_sig, const double *gam_tau,
                            const int32_t *progress, const uint64_t *span, int stat_first, int64_t *ticket,
                            const double **stats_area);
/* segments regenerated on the device so far, chains submitted as rows */
int fokl_dchain_stream_stats(fokl_dchain *engine, int64_t *segments_made, int64_t *rows_jobs);
int fokl_dchain_poll(fokl_dchain *engine, int64_t ticket);
int fokl_dchain_flush(fokl_dchain *engine);   /* issue what is queued now: nothing more is coming for a while */
int fokl_dchain_wait(fokl_dchain *engine, int64_t ticket, double *stats_out);
int fokl_dchain_fetch_w(fokl_dchain *engine, int64_t ticket, double *w_out);
int fokl_dchain_release(fokl_dchain *engine, int64_t ticket);
/* The same without waiting: 1 = the slot is free (now or before), 0 = the chain has not run yet. */
int fokl_dchain_try_release(fokl_dchain *engine, int64_t ticket);
/* seconds the dispatcher spent issuing work, number of chains issued, number of recursion launches (chains whose
 * tapes are ready together go out as one launch: FOKL_DCHAIN_BATCH chains or FOKL_DCHAIN_DELAY_US after the oldest was
 * queued, at once when somebody waits for a result); `staged` = chains whose tape was not in page-locked memory and
 * went through copy calls + a device staging buffer instead of being read in place */
int fokl_dchain_stats(fokl_dchain *engine, double *busy_seconds, int64_t *issued, int64_t *launches, int64_t *staged);
/* chains, among those seen to have run (wait, poll, fetch or release), that the segmented recursion ran a second time in
 * one piece: each costs a one-wavefront chain on top of the segmented one */
int fokl_dchain_recuts(fokl_dchain *engine, int64_t *recuts);

/* ---- G2 on the device: eigen-decompositions of candidate models' XtX sub-blocks -------------------------------------
 * Replaces, for models of up to FOKL_DSPECTRAL_MAX_COLUMNS columns, the scipy.linalg.eigh call of FoKLRoutines.py:1499
 * and the products of FR:1502-1504 that hang on it (on the host: fokl_pool_submit_spectral, LAPACK dsyevr on a thread).
 * One workgroup per matrix runs a cyclic Jacobi iteration on the matrix in LDS, one wavefront per eigenvector column
 * replays its rotations (csrc/fokl_spectral_device.inc).
 *
 * fokl_dspectral_submit copies the sub-block XtX[idx][idx], Xty = gram[idx][ycol], the ones row gram[0][idx] and
 * gram[0][ycol], gram[ycol][ycol] (gram: [ld][ld] row-major, symmetric, column 0 the ones column) into page-locked memory
 * of the engine -- the caller's array is not referenced after the call -- and stages the job; launch != 0 launches what is
 * staged at once, 0 leaves it for fokl_dspectral_flush (several jobs become one grid) or for the first poll / wait of any
 * of them.  *result is the job's page-locked result area, owned by the engine until fokl_dspectral_release:
 *   lamb [p1] ascending | qty = Q'Xty [p1] | betahat [p1] | Qt [p1][p1] (row j = eigenvector j) | sum r, sum r^2 |
 *   sweeps, rotations, seconds on the device, 1 if the sweeps did not converge | the job's ticket (as a double)
 * the ticket stored last with system-wide release semantics: a caller may poll that word.  Eigenvector signs follow
 * engine.eigh_canonical (largest-magnitude component positive, first on ties) unless fokl_dspectral_set_signs(e, 0).
 * fokl_dspectral_poll: 1 = has run, 0 = not yet, < 0 = -error.  fokl_dspectral_wait: FOKL_OK, or FOKL_ERR_NUMERIC when
 * the sweeps did not converge.  fokl_dspectral_release waits for a job still in flight; idempotent. */
#define FOKL_DSPECTRAL_MAX_COLUMNS 192
int fokl_dspectral_create(int device, fokl_dspectral **out);
void fokl_dspectral_destroy(fokl_dspectral *engine);
int fokl_dspectral_max_columns(void);
int fokl_dspectral_set_signs(fokl_dspectral *engine, int canonical);
int fokl_dspectral_submit(fokl_dspectral *engine, const double *gram, int ld, const int32_t *idx, int p1, int ycol,
                          int launch, int64_t *ticket, double **result);
int fokl_dspectral_flush(fokl_dspectral *engine);
int fokl_dspectral_poll(fokl_dspectral *engine, int64_t ticket);
int fokl_dspectral_wait(fokl_dspectral *engine, int64_t ticket);
int fokl_dspectral_release(fokl_dspectral *engine, int64_t ticket);
int fokl_dspectral_stats(fokl_dspectral *engine, int64_t *submitted, int64_t *launches);
/* Page-locked host memory for tapes: the device reads such a tape in place (no copy calls on the dispatcher). */
int fokl_host_alloc(size_t bytes, void **out);
int fokl_host_free(void *ptr);

/* ------------------------------------------------------------------------------------------------------ */
/* Optimising a fitted model over its posterior (csrc/fokl_optimize_device.inc; fokl_gpy_amd/optimize.py)     */
/* ------------------------------------------------------------------------------------------------------ */

/*
 * n_draws x n_starts box-constrained local solves of a 'Bernoulli Polynomials' model at once, one lane per solve:
 *     minimise  sign * ( betas[e][0] + sum_t betas[e][t + 1] * prod_j phi_{mtx[t][j]}(x_j) )   over  lo <= x <= hi
 * for every draw e from every start s, in NORMALISED coordinates (the caller de-normalises).  Host memory, row-major:
 *   mtx    [n_terms, n_inputs]   orders, 0 = the input is not in the term
 *   betas  [n_draws, n_terms + 1]
 *   table  [n_basis, width]      row o - 1 holds the o + 1 coefficients of order o, constant first (fokl_upload's
 *                                Bernoulli layout); an order needs o <= n_basis and o < width
 *   lo, hi [n_inputs]            the box; lo[j] == hi[j] fixes input j
 *   starts [n_starts, n_inputs]  clipped to the box
 *   sign   +1 minimises the model, -1 maximises it;  tol  bound on max_j |P(x - g)_j - x_j| (P clips to the box)
 * Outputs: x [n_draws, n_starts, n_inputs] the end points, f [n_draws, n_starts] the MODEL's value there,
 * iterations and status [n_draws, n_starts]: 0 converged, 1 iteration limit (max_iter), 2 non-finite value or gradient,
 * 3 stalled (no trial point of the line search, Newton or steepest descent, decreases the value).
 * The iteration -- projected Newton on the active set, Cholesky modified in place where the Hessian is not positive
 * definite, halving along the projection arc under an Armijo test with a rounding allowance -- is stated in numpy by
 * optimize.solve_host, which the kernel is tested against: same results up to the rounding of differently ordered sums.
 * Limits (FOKL_ERR_ARG with a text, nothing is launched): at most 16 inputs; 3 x distinct (input, order) factors +
 * n_inputs (n_inputs + 1) / 2 + 3 n_inputs <= 288 (a solve's values live in LDS, 64 solves wide, within 144 KB); orders
 * within the table; lo <= hi, finite; n_draws * n_starts <= 1 048 576; sign +-1, max_iter >= 0, tol >= 0.
 * Needs a context, no dataset: everything it uses is uploaded by the call and freed before it returns; the context's
 * dataset, slots and pending launches are left alone (it may be called between fits).  One launch for all solves.
 * Kernel time: FOKL_K_OPTIMIZE.  Blocking.
 */
int fokl_model_optimize(fokl_ctx *ctx, int n_inputs, int n_terms, const int32_t *mtx, int n_draws, const double *betas,
                        const double *table, int n_basis, int width, const double *lo, const double *hi, int n_starts,
                        const double *starts, double sign, int max_iter, double tol, double *x, double *f,
                        int32_t *iterations, int32_t *status);

/* ------------------------------------------------------------------------------------------------------ */
/* Constrained optimisation over a system of models (csrc/fokl_optimize_system_device.inc; optimize.py)       */
/* ------------------------------------------------------------------------------------------------------ */

/*
 * n_draws x n_starts constrained local solves over a SYSTEM of 'Bernoulli Polynomials' models at once, one lane per
 * solve, in the COMMON normalised coordinates z [n_vars] of optimize.optimize_system (which assembles all of this):
 *     minimise  sign * objective(z)   over  lo <= z <= hi   subject to the constraints below,
 * by a bound-constrained augmented Lagrangian whose inner iteration is fokl_model_optimize's projected Newton step.
 * Model k reads shift + slope * z[var_of] at each of its inputs.  Host memory, row-major, the models' pieces one after
 * the other:
 *   n_inputs, n_terms [n_models]
 *   mtx      model k's [n_terms[k], n_inputs[k]] orders (0 = the input is not in the term)
 *   var_of, shift, slope   per model and input: the variable it reads (each at most once per model) and the map
 *   betas    [n_draws, sum_k (n_terms[k] + 1)]   a draw's row: every model's coefficients side by side, constant first
 *   table    [n_basis, width]   as for fokl_model_optimize
 *   lo, hi   [n_vars] the box, lo[v] == hi[v] fixes a variable;  starts [n_starts, n_vars], clipped to the box
 *   objective: model obj_model's output (obj_var = -1), or obj_offset + obj_span * z[obj_var] (obj_model = -1)
 *   sign     +1 minimises, -1 maximises
 *   constraints, ordered by model, per model at most one range and then at most one tie:
 *     con_model [n_con]   the model whose output r the constraint reads
 *     con_var   [n_con]   -1: a range;  v >= 0: a tie, r = output - (offset + span * z[v]), an equality at 0
 *     con_par   [n_con, 5]   lo, hi, scale, offset, span: lo <= r <= hi with -inf / +inf for a missing side, lo == hi an
 *                            equality; residuals are divided by scale (> 0) before ctol applies
 *   tol      bound on the projected gradient of the merit function;  ctol  bound on the scaled residuals (for an
 *            inequality that holds: on the distance of its multiplier from complementarity)
 * Outputs: x [n_draws, n_starts, n_vars] end points, f [.., ..] the OBJECTIVE there, violation [.., ..] the largest
 * scaled residual, y [.., .., n_models] every model's value, multipliers [.., .., n_con] d merit / d r of every
 * constraint (first-order estimates: >= 0 upper side, <= 0 lower side, 0 inactive), iterations and status: 0 converged,
 * 1 iteration limit, 2 non-finite, 3 stalled, 4 infeasible (ended with violation > ctol).  An iteration is a Newton step
 * or a multiplier / penalty update; max_iter counts both.  The statement the kernel is tested against is
 * optimize.solve_system_host.
 * Limits (FOKL_ERR_ARG with a text, nothing is launched): n_vars <= 16; n_models <= 8; 3 x (most distinct (input,
 * order) factors of one model) + n_vars (n_vars + 1) / 2 + 3 n_vars + 2 n_models + 2 n_con <= 288 (a solve's values
 * live in LDS, 64 solves wide, within 144 KB); orders within the table; lo <= hi, finite; variable and model indices in
 * range; n_draws * n_starts <= 1 048 576; sign +-1; max_iter, tol, ctol >= 0.
 * Needs a context, no dataset: everything it uses is uploaded by the call and freed before it returns; the context's
 * dataset, slots and pending launches are left alone.  The solves are sliced over launches of at most
 * 4 194 304 / max_iter solves (whole wavefronts, at least one), so that no launch is asked for more solve-iterations
 * than that.  Kernel time: FOKL_K_OPTIMIZE_SYSTEM (one entry per launch).  Blocking.
 */
int fokl_system_optimize(fokl_ctx *ctx, int n_vars, int n_models, const int32_t *n_inputs, const int32_t *n_terms,
                         const int32_t *mtx, const int32_t *var_of, const double *shift, const double *slope, int n_draws,
                         const double *betas, const double *table, int n_basis, int width, const double *lo,
                         const double *hi, int n_starts, const double *starts, int obj_model, int obj_var,
                         double obj_offset, double obj_span, double sign, int n_con, const int32_t *con_model,
                         const int32_t *con_var, const double *con_par, int max_iter, double tol, double ctol, double *x,
                         double *f, double *violation, double *y, double *multipliers, int32_t *iterations,
                         int32_t *status);

/* ------------------------------------------------------------------------------------------------------ */
/* The optimisers' Newton step, one iteration at a time: traces and launch reports (tests; optimize.py)       */
/* ------------------------------------------------------------------------------------------------------ */

#define FOKL_OPTIMIZE_REPORT_LEN 9
/* out[0] of fokl_optimize_report / fokl_system_optimize_report: the instantiation that ran */
enum {
    FOKL_OPTIMIZE_NONE = 0,       /* no call yet, or the last one was refused or failed: nothing to report */
    FOKL_OPTIMIZE_UNIFORM = 1,    /* n_starts a multiple of 64: a wavefront belongs to one draw, scalar coefficient loads */
    FOKL_OPTIMIZE_PER_LANE = 2    /* every lane reads its own draw's row */
};

/*
 * fokl_model_optimize / fokl_system_optimize with one more result: what iteration `trace_iteration` (0 = the first pass)
 * of every solve saw and decided, written by the TRACE instantiation of the SAME kernel body the product launches
 * (the tracing statements are compiled away in the product's instantiations).  Everything else -- arguments, checks,
 * results, launches -- is the product entry point's: both run one host function.
 * trace [n_draws * n_starts, stride] doubles, host memory; flags and counts are stored as doubles.  With m = n_inputs (or
 * n_vars), h = m (m + 1) / 2, a row is
 *   [0]  running: 1 the solve was running when the iteration began, 0 it had stopped before (or its whole wavefront had)
 *   [1] F  [2] noise  [3] pg  [4] active (bit j: coordinate j)  [5] status after the iteration's tests (-1: runs on)
 *   [6] stepping  [7] use_steepest  [8] trial points evaluated while searching  [9] alpha  [10] failed
 *   [11] steepest for the next iteration  [12] status at the iteration's exit (-1: runs on)
 *   then x_in [m], g [m], H [h] before the factorisation, the factor [h], d [m] after the fall-back select and the
 *   scaling, Ft [31] of the trial points (NaN beyond those evaluated), x_out [m]:  stride = 13 + 4 m + 2 h + 31;
 *   the system's rows go on with ev [K], nz [K], lam [2 C], rho, inner, target, viol, measure, update, good at the entry
 *   and lam [2 C], rho, inner, target at the exit:  stride = 13 + 4 n + 2 h + 31 + 2 K + 4 C + 10.
 * What a row does not get stays NaN: everything but running for a solve whose wavefront ended before the iteration;
 * everything but running, both statuses, x_in and x_out (= x_in) for a solve that had stopped; the step's values when
 * the wavefront ended at this iteration's tests.  Values of a lane that is not `stepping` are what the kernel computed
 * and dropped.
 */
int fokl_model_optimize_trace(fokl_ctx *ctx, int n_inputs, int n_terms, const int32_t *mtx, int n_draws,
                              const double *betas, const double *table, int n_basis, int width, const double *lo,
                              const double *hi, int n_starts, const double *starts, double sign, int max_iter, double tol,
                              double *x, double *f, int32_t *iterations, int32_t *status, int trace_iteration,
                              double *trace);
int fokl_system_optimize_trace(fokl_ctx *ctx, int n_vars, int n_models, const int32_t *n_inputs, const int32_t *n_terms,
                               const int32_t *mtx, const int32_t *var_of, const double *shift, const double *slope,
                               int n_draws, const double *betas, const double *table, int n_basis, int width,
                               const double *lo, const double *hi, int n_starts, const double *starts, int obj_model,
                               int obj_var, double obj_offset, double obj_span, double sign, int n_con,
                               const int32_t *con_model, const int32_t *con_var, const double *con_par, int max_iter,
                               double tol, double ctol, double *x, double *f, double *violation, double *y,
                               double *multipliers, int32_t *iterations, int32_t *status, int trace_iteration,
                               double *trace);

/*
 * What the last fokl_model_optimize(_trace) / fokl_system_optimize(_trace) call on `ctx` ran, out [9] (host values, no
 * launch): the instantiation (FOKL_OPTIMIZE_*), the grid (workgroups = wavefronts; the system's: of its first launch),
 * lds_bytes, whether the attribute that allows more than 64 KB of LDS was set, slots (distinct (input, order) factors;
 * the system's: of its largest model), side-list entries, solves, launches, 1 if it was a trace.  All zeros after a call
 * that was refused or failed.
 */
int fokl_optimize_report(const fokl_ctx *ctx, int64_t *out);
int fokl_system_optimize_report(const fokl_ctx *ctx, int64_t *out);

/* ------------------------------------------------------------------------------------------------------ */
/* Embedded GPs: HMC chains of GPs inside a traced equation (csrc/fokl_embedded_device.inc; embedded.py)     */
/* ------------------------------------------------------------------------------------------------------ */

/*
 * n_chains Hamiltonian Monte Carlo chains, ONE WORKGROUP PER CHAIN and the whole chain in one launch, of the model
 *     data_i = equation(g_0i .. g_{K-1}i; columns) + noise,   g_k = X beta_k,   q = (beta_0 .. beta_{K-1}, ln sigma^2)
 * over the dataset uploaded to the context (fokl_upload; data is FOKL_SLOT_Y).  X is the n_coef basis columns in
 * term_slots (intercept first: FOKL_SLOT_ONES, then what fokl_build_terms built), shared by the K GPs.
 *   col_slots [n_cols]     slots holding the equation's known columns (fokl_write_slot)
 *   ops       [n_ops, 3]   the tape in single-assignment form: (opcode, a, b).  Opcodes 0 add, 1 sub, 2 mul, 3 div
 *                          (binary); 4 neg, 5 exp, 6 log, 7 sqrt, 8 square, 9 reciprocal (unary, b ignored); 10 power
 *                          with a constant exponent (b a constant).  An operand is (kind << 8) | index: kind 0 a value
 *                          (index k < K is GP k, index K + o the result of operation o, which must precede its use),
 *                          kind 1 column `index`, kind 2 constant `index`.
 *   consts    [n_consts]   result: the operand (kind 0) that is the equation's value
 *   q0        [n_chains, D] start states, D = K n_coef + 1, or NULL for all ones
 *   eps0      > 0: the first step size (no step search at the start); 0: find_reasonable_epsilon
 *   adapt     non-zero: the step size is rescaled every 50 draws by the window's acceptance count and the inverse mass
 *             becomes the per-parameter variance of states 401 .. 500 after draw 500 (if 5 of those draws moved)
 * Random numbers: Philox 4x32-10 keyed by (seed, chain), counter (draw, purpose, index) -- fokl_embedded_rng below.
 * Outputs (host): states [n_chains, draws + 1, D] (row 0 the start), potential U and accept flags [n_chains, draws + 1],
 * eps_hist [n_chains, draws / 50] the step size after every window, inv_mass [n_chains, D], eps_final [n_chains],
 * status [n_chains, 2]: (0 ok | 1 no step: the capped step search found no finite step, the rest of the chain is NaN;
 * 1 if the mass update fired).  Optional (may be NULL): grad0 [n_chains, D] dU/dq at the start, proposal
 * [n_chains, D + 1] the last transition's proposal and its potential.
 * The statement the kernel is tested against is embedded.full_sample_host.
 * Limits (FOKL_ERR_ARG with a text, nothing is launched): K in 1 .. 8; n_cols <= 16; n_ops <= 32; n_consts <= 64;
 * D <= 257; rows x n_coef <= 4 194 304 (all chains stream the same X from the last-level cache); n_chains <= 4096;
 * draws <= 1 000 000; leapfrog in 1 .. 1000; a well-formed tape; slots in range.  The dataset, its slots and pending
 * launches are left alone; per-chain scratch is allocated by the call and freed before it returns.  Blocking.
 */
int fokl_embedded_hmc(fokl_ctx *ctx, int n_gps, int n_coef, const int32_t *term_slots, int n_cols,
                      const int32_t *col_slots, int n_ops, const int32_t *ops, int n_consts, const double *consts,
                      int32_t result, int n_chains, int draws, int leapfrog, uint32_t seed, const double *q0, double eps0,
                      int adapt, double *states, double *potential, int32_t *accepted, double *eps_hist, double *inv_mass,
                      double *eps_final, int32_t *status, double *grad0, double *proposal);

/*
 * The launch plan fokl_embedded_hmc chooses for a tape of n_ops operations over n_gps GPs, by the expression it launches
 * with: *threads the workgroup's size -- 256 while the n_gps + n_ops value and adjoint slots of 256 threads fit the 160 KB
 * of LDS beside the chain's state (up to 34 slots), 128 above that -- and *lds_bytes the dynamic LDS it asks for.  No
 * device, no context; FOKL_ERR_ARG outside 1 .. 8 GPs or 0 .. 32 operations.
 */
int fokl_embedded_plan(int n_gps, int n_ops, int *threads, size_t *lds_bytes);

/*
 * out[j], j < count: the numbers chain `chain` of a run seeded `seed` draws at `draw` for `purpose` -- 0 the momentum of
 * transition `draw` (standard normals, one per parameter), 1 its accept uniform (j = 0), 2 the momentum of the step
 * search that runs at `draw` (0 at the start, 500 after the mass update); and those of fokl_resample_chains, whose `draw`
 * is the Gibbs iteration: 3 the normals of the eigen-coordinates j, 4 / 5 the normal / uniform of attempt j of sigma^2's
 * gamma variate, 6 / 7 of tau^2's, 8 the uniforms behind a dispersed start (draw 0; j = 0 sigma^2, 1 tau^2).
 * Host code, no device (csrc/fokl_philox.h).
 */
int fokl_embedded_rng(uint32_t seed, uint32_t chain, uint32_t draw, int purpose, int count, double *out);

/* ------------------------------------------------------------------------------------------------------ */
/* Resampling a fitted model's posterior (csrc/fokl_resample_device.inc; fokl_gpy_amd/resample.py)           */
/* ------------------------------------------------------------------------------------------------------ */

#define FOKL_RESAMPLE_REPORT_LEN 10
#define FOKL_RESAMPLE_MAX_COLUMNS 768      /* 12 eigen-coordinates per lane: FOKL_DCHAIN_MAX_COLUMNS' bar */
#define FOKL_RESAMPLE_ATTEMPT_CAP 64       /* Marsaglia-Tsang attempts per gamma variate unless the call says otherwise */
#define FOKL_RESAMPLE_SEGMENTS 3           /* per-chain sums: first half, second half, the odd last iteration */

/*
 * `chains` independent chains of the recursion fokl_gibbs_chain documents (include/fokl_hip.h), burnin + draws iterations
 * each, in the eigenbasis (lamb, qty [p1]; astar, atau_star, b, btau, dtd as there), chain c started at sigsqd0[c],
 * tausqd0[c].  Random numbers: Philox 4x32-10 keyed by (seed, c), counter (iteration, purpose, index) -- fokl_embedded_rng's
 * purposes 3 .. 7; the gamma variates by Marsaglia-Tsang (shapes >= 1), at most `attempt_cap` attempts each (0: the default).
 * One wavefront per chain, `chains_per_group` chains per workgroup (0: the default, 4; a test hook: the results do not
 * depend on it), no atomics: the same arguments give the same bits.
 * Outputs (host): with rows kept, iteration burnin + r thin of chain c is row c kept + r, kept = ceil(draws / thin), of
 *   w_out [chains kept, p1], sig_out, tau_out [chains kept] (the iteration's new sigsqd, tausqd) and attempts_out
 *   [chains kept] (attempts of its two gamma variates); all four NULL: no rows.
 *   sums_out [chains, 3, 2, p1 + 2]: over the first half (draws / 2 iterations), the second half and the odd last of the
 *   post-burn-in iterations, the sums and the sums of squares of w_i - shift[i] (i < p1), sigsqd (p1) and tausqd (p1 + 1),
 *   each accumulated in iteration order.
 *   counts_out [chains, 4]: the first flagged iteration or -1, why (1: bstar < 0, sigsqd is NaN as FR:1538-1541 leaves
 *   it; 2: a gamma variate met the attempt cap and is NaN), attempts in all, the most attempts of one variate.  A flagged
 *   chain runs on, NaN from there; the other chains are not affected.
 * Refused (FOKL_ERR_ARG with a text, nothing is launched): p1 > FOKL_RESAMPLE_MAX_COLUMNS; a shape below 1; rows that do
 * not fit the device's free memory.  The dataset, its slots and pending launches are left alone.  Blocking.
 * The statement the kernel is tested against is resample.resample_host.  Kernel time: FOKL_K_RESAMPLE.
 */
int fokl_resample_chains(fokl_ctx *ctx, int p1, const double *lamb, const double *qty, const double *shift,
                         double astar, double atau_star, double b, double btau, double dtd, int chains,
                         const double *sigsqd0, const double *tausqd0, int burnin, int draws, int thin, uint32_t seed,
                         int chains_per_group, int attempt_cap, double *w_out, double *sig_out, double *tau_out,
                         int32_t *attempts_out, double *sums_out, int64_t *counts_out);

/*
 * The last fokl_resample_chains call on `ctx`, out [FOKL_RESAMPLE_REPORT_LEN] (host):
 *   out[0]  the instance that ran: eigen-coordinates per lane (1, 2, 3, 4, 6, 8 or 12); zeros after a refused call
 *   out[1]  chains     out[2]  iterations per chain (burn-in included)     out[3]  wavefronts (chains) per workgroup
 *   out[4]  Marsaglia-Tsang attempts in all     out[5]  the most any variate needed     out[6]  kernel microseconds
 *   out[7]  the grid     out[8]  flagged chains     out[9]  rows kept per chain (the call's kept, also without rows)
 */
int fokl_resample_report(const fokl_ctx *ctx, int64_t *out);

/* ------------------------------------------------------------------------------------------------------ */
/* A robust posterior: Student-t noise and row weights (csrc/fokl_robust_device.inc; fokl_gpy_amd/robust.py)  */
/* ------------------------------------------------------------------------------------------------------ */

#define FOKL_ROBUST_REPORT_LEN 16
#define FOKL_ROBUST_MAX_COLUMNS 127        /* P + 1: [1 | X | y] fills eight 16-column blocks of the weighted Gram */

/*
 * The model: y_i = x_i . beta + eps_i, eps_i | lam_i ~ N(0, sigsqd / (w_i lam_i)), lam_i ~ Gamma(nu / 2, rate nu / 2); nu
 * fixed (INFINITY: lam = 1), w given.  Iteration k of a chain is a row pass, a reduce and a step (robust.py states every
 * operation).  Random numbers: Philox 4x32-10 keyed by (seed, chain), counter (iteration, purpose + 16 attempt, index, 4)
 * (csrc/fokl_philox.h, ROB_PURPOSE_*; fokl_robust_rng below).  X_i: the columns `slots`, nc = P + 1 of them, of the
 * uploaded rows; y: FOKL_SLOT_Y.  weights [n_weights] host, n_weights = the uploaded rows, or NULL: ones.
 *
 * fokl_robust_pass: one row pass.  At iteration 0 or nu = INFINITY lam = 1 (beta and sigsqd are not read); otherwise
 * r_i = y_i - x_i . beta, lam_i = g_i / ((nu + w_i r_i^2 / sigsqd) / 2), g_i a standard gamma of shape (nu + 1) / 2 by
 * Marsaglia-Tsang, at most attempt_cap attempts (0: the default, FOKL_RESAMPLE_ATTEMPT_CAP), NaN beyond.
 *   G_out [nc + 1, nc + 1] = [X|y]' diag(w lam) [X|y], exactly symmetric; lam_out [rows], attempts_out [rows], or NULL.
 * robust_pass_kernel accumulates the upper block triangle of G on v_mfma_f64_16x16x4_f64 per workgroup of four wavefronts
 * over a range of rows that depends on the number of rows alone; robust_reduce_kernel sums the workgroups' partials in
 * their order.  No atomics: the same arguments give the same bits.
 */
int fokl_robust_pass(fokl_ctx *ctx, const int32_t *slots, int nc, const double *weights, int64_t n_weights, const double *beta,
                     double sigsqd, double nu, uint32_t seed, uint32_t chain, uint32_t iteration, int attempt_cap,
                     double *G_out, double *lam_out, int32_t *attempts_out);

/*
 * fokl_robust_step: one step on a given G [nc + 1, nc + 1] (host; symmetric: its upper triangle is read), needs no dataset:
 * A = G_xx + I / tausqd = L L' without pivoting, L u = G_xy, L' beta = u + sqrt(sigsqd) z; S = G_yy - 2 beta . G_xy +
 * beta' G_xx beta; bstar = b + (S + beta . beta / tausqd) / 2; sigsqd' = 1 / Gamma(astar, 1 / bstar); tausqd' = 1 /
 * Gamma(atau_star, 1 / (beta . beta / (2 sigsqd') + btau)).
 *   beta_out [nc]; state_out [2] = sigsqd', tausqd'; counts_out [4] = `iteration` if the step flagged else -1, why (1: bstar
 *   < 0; 2: a gamma variate met the attempt cap, or G is NaN because a row of the pass did; 3: a pivot was not positive),
 *   the attempts of the two variates, the most of one.  A flagged step's outputs are NaN.
 */
int fokl_robust_step(fokl_ctx *ctx, int nc, const double *G, double sigsqd, double tausqd, double astar, double atau_star,
                     double b, double btau, uint32_t seed, uint32_t chain, uint32_t iteration, int attempt_cap,
                     double *beta_out, double *state_out, int64_t *counts_out);

/*
 * fokl_robust_chains: `chains` chains of burnin + draws iterations, chain c keyed by chain_ids[c] (NULL: c) and started at
 * sigsqd0[c], tausqd0[c]; three launches per iteration queued on the context's stream, no host round trip between them
 * (nu = INFINITY: the pass and the reduce run once, G does not change).  Outputs (host) as fokl_resample_chains', with
 * betas_out [chains kept, nc] in place of w_out, attempts_out [chains kept] int64 (the rows' variates included), sums_out
 * [chains, 3, 2, nc + 2] of beta - shift | sigsqd | tausqd, counts_out [chains, 4] as fokl_robust_step's; and lam_sum_out
 * [chains, rows] (or NULL): the sum of lam_i over the passes of the post-burn-in iterations.  A flagged chain runs on, NaN
 * from there; the other chains are not affected; chain c does not depend on how many chains run with it.
 * Refused (FOKL_ERR_ARG with a text, nothing is launched; the dataset, its slots and pending launches are left alone):
 * nc > FOKL_ROBUST_MAX_COLUMNS; a slot outside the table; n_weights that is not the number of rows; nu < 1 or NaN; a shape
 * below 1; rows, row weights and partial Grams beyond the device's free memory (the environment's FOKL_ROBUST_FREE_BYTES,
 * if set, caps what counts as free).  Kernel time: FOKL_K_ROBUST, three launches per iteration.  Blocking.
 */
int fokl_robust_chains(fokl_ctx *ctx, const int32_t *slots, int nc, const double *weights, int64_t n_weights, double nu,
                       double astar, double atau_star, double b, double btau, const double *shift, int chains,
                       const int32_t *chain_ids, const double *sigsqd0, const double *tausqd0, int burnin, int draws, int thin,
                       uint32_t seed, int attempt_cap, double *betas_out, double *sig_out, double *tau_out,
                       int64_t *attempts_out, double *sums_out, int64_t *counts_out, double *lam_sum_out);

/*
 * The last fokl_robust_pass / _step / _chains call on `ctx`, out [FOKL_ROBUST_REPORT_LEN] (host); zeros after a refused call:
 *   out[0]  workgroups of the pass per chain = partial Grams (0: a step alone)     out[1]  chains (the grid's second dimension)
 *   out[2]  doubles of one partial     out[3]  LDS bytes of the pass     out[4]  LDS bytes of the step
 *   out[5]  columns of [X|y]     out[6]  16-column blocks     out[7]  iterations     out[8]  rows kept per chain
 *   out[9]  Marsaglia-Tsang attempts in all     out[10] flagged chains
 *   out[11 .. 13]  microseconds of the pass, the reduce and the step, summed over out[14] iterations (the last ones of a
 *   run, 64 at most, timed launch by launch)     out[15] microseconds of the whole run
 */
int fokl_robust_report(const fokl_ctx *ctx, int64_t *out);

/*
 * The numbers of indices first .. first + count - 1 of (seed, chain, iteration, purpose, attempt): uniforms for the purposes
 * 1, 4, 6, normals otherwise (csrc/fokl_philox.h: ROB_PURPOSE_*).  Host code, no device.
 */
int fokl_robust_rng(uint32_t seed, uint32_t chain, uint32_t iteration, int purpose, int attempt, uint32_t first, int64_t count,
                    double *out);

/* ------------------------------------------------------------------------------------------------------ */
/* What a prediction ran (csrc/fokl_predict.inc)                                                             */
/* ------------------------------------------------------------------------------------------------------ */

/* out[0] of fokl_predict_report */
enum {
    FOKL_PREDICT_NONE = 0,        /* no call yet, or the last one was refused or failed: nothing to report */
    FOKL_PREDICT_VALU_LDS = 1,    /* predict_kernel, order-statistic lists in LDS (or none: mean only) */
    FOKL_PREDICT_VALU_GLOBAL = 2, /* predict_kernel, lists in device memory (klo > 128, or no room next to the basis values) */
    FOKL_PREDICT_MFMA = 3         /* predict_mfma_kernel */
};

/*
 * The last fokl_predict call on `ctx`, out [6] (host):
 *   out[0]  the kernel it launched (above); a call that returned an error leaves FOKL_PREDICT_NONE and zeros
 *   out[1]  1 if the model was too wide for its rows' basis values to sit in LDS and the VALU kernel read them from the
 *           columns (about 300 terms and more), else 0
 *   out[2]  the launch's grid (workgroups = wavefronts)
 *   out[3]  the row tiles it covered: 16-row tiles of predict_mfma_kernel, 64-row blocks of predict_kernel; more tiles
 *           than workgroups means the kernel's grid-stride loop went round again
 *   out[4]  tiles predict_mfma_kernel counted as processed (= out[3] if every one was visited once), 0 for predict_kernel
 *   out[5]  those among them whose filter pass did not yield the bounds and which went through the exact fallback pass
 *           (same numbers at about a third of the speed), 0 for predict_kernel.  (= out[4] with a coefficient that is not finite: the
 *           filter's moments are NaN.  Rows whose mean is not finite are then written again by predict_kernel's repair pass,
 *           which counts their NaN predictions -- include/fokl_hip.h, fokl_predict; this report stays the first kernel's)
 * Host values and two device counters copied back with the results: no launch, no synchronisation of its own.
 */
int fokl_predict_report(const fokl_ctx *ctx, int64_t *out);

/* ------------------------------------------------------------------------------------------------------ */
/* A population through every posterior draw (csrc/fokl_population.inc; fokl_gpy_amd/population.py)          */
/* ------------------------------------------------------------------------------------------------------ */

/* out[0] of fokl_population_report: where a wavefront's draw coefficients lived */
enum {
    FOKL_POPULATION_NONE = 0,      /* no call yet, or the last one was refused or failed */
    FOKL_POPULATION_REGISTERS = 1, /* in registers for the whole launch (at most 128 columns, padded to 4) */
    FOKL_POPULATION_TABLE = 2      /* read from the transposed table one k-step ahead (wider models) */
};
#define FOKL_POPULATION_REPORT_LEN 8
#define FOKL_POPULATION_MAX_CUTS 32

/*
 * The transpose of fokl_predict: y[row][d] = sum_k column(slots[k])[row] * betas[d][k] over the uploaded rows, reduced
 * over the ROWS for every draw d (fokl_predict reduces over the draws for every row).  Host memory, row-major:
 *   slots [nc], betas [draws, nc]   as for fokl_predict; any nc >= 1, any draws >= 1
 *   shift [draws]                   c_d, a value near draw d's mean: the second moment is accumulated about it
 *   cuts  [draws, n_cuts]           per-draw cut points, 0 <= n_cuts <= FOKL_POPULATION_MAX_CUTS (may be NULL if 0)
 *   with_data                       non-zero: also the residuals e = data - y against the uploaded y (FOKL_SLOT_Y)
 * Outputs:
 *   moments_out [draws, 6]          sum(y - c), sum((y - c)^2), min y, max y, sum(e), sum(e^2) (the last two 0 without data)
 *   above_out   [draws, n_cuts]     the number of rows with y > cuts[d][k], strictly (may be NULL if n_cuts is 0)
 * One launch of population_kernel on v_mfma_f64_16x16x4_f64 (a lane keeps the accumulators of one draw in registers;
 * each (row chunk, draw) leaves one record) and one of population_reduce_kernel, which adds the records in the order
 * of the chunks: no floating-point atomics, the same arguments give the same bits.  y itself is never stored.
 * Refused (FOKL_ERR_ARG, "every coefficient must be finite", before anything is allocated or launched): a NaN or infinite
 * entry of betas.
 * Kernel time: FOKL_K_POPULATION (both launches).  Blocking.
 */
int fokl_population_stats(fokl_ctx *ctx, const int32_t *slots, int nc, const double *betas, int draws,
                          const double *shift, const double *cuts, int n_cuts, int with_data, double *moments_out,
                          int64_t *above_out);

/*
 * The last fokl_population_stats call on `ctx`, out [FOKL_POPULATION_REPORT_LEN] (host):
 *   out[0]  where the coefficients lived (above); zeros after a call that returned an error
 *   out[1]  the grid (workgroups of 8 wavefronts = 128 draws): row chunks, rounded up to 8, x draw blocks
 *   out[2]  draw blocks     out[3]  row chunks with rows     out[4]  16-row tiles per chunk     out[5]  row tiles
 *   out[6]  dynamic LDS bytes     out[7]  pieces the columns were walked in per tile (above 1: more than 1024 columns)
 * Host values noted while enqueuing: no launch, no synchronisation.
 */
int fokl_population_report(const fokl_ctx *ctx, int64_t *out);

/* ------------------------------------------------------------------------------------------------------ */
/* Scoring a fitted model pointwise: WAIC and PSIS-LOO (csrc/fokl_score_device.inc; fokl_gpy_amd/score.py)   */
/* ------------------------------------------------------------------------------------------------------ */

/* out[0] of fokl_score_report: the instance of score_kernel that ran */
enum {
    FOKL_SCORE_NONE = 0,      /* no call yet, or the last one was refused or failed */
    FOKL_SCORE_WAIC = 1,      /* want_loo = 0: lppd, ll_mean, p_waic only, no list in LDS */
    FOKL_SCORE_WAIC_LOO = 2   /* also the top-(M + 1) list, the Pareto fit and elpd_loo */
};
/* the last entry of fokl_score_report and of fokl_predictive_report: the noise instance of the kernel that ran */
enum {
    FOKL_NOISE_GAUSSIAN = 0,           /* N(mu, sigsqd): the instance of fokl_score_rows / fokl_predictive_rows */
    FOKL_NOISE_GAUSSIAN_WEIGHTED = 1,  /* N(mu, sigsqd / w_i) */
    FOKL_NOISE_STUDENT = 2             /* t_nu(mu, scale sqrt(sigsqd / w_i)), weighted or not */
};
#define FOKL_SCORE_REPORT_LEN 8
#define FOKL_SCORE_STATS 8
#define FOKL_SCORE_MIN_DRAWS 25      /* PSIS needs a tail of at least 5 draws */
/* Entries (M + 1) of a row's list of largest log ratios in LDS: 512 x 16 rows x 8 B = 64 KiB of the compute unit's 160 KiB,
 * which leaves room for the basis values of a 16-row tile of a model of 750 columns next to it.  M = min(E / 5,
 * ceil(3 sqrt(E))) <= 511 allows E <= 29 013 draws. */
#define FOKL_SCORE_MAX_TAIL 512

/*
 * ll[i][d] = -log(2 pi sigsqd[d]) / 2 - (y_i - X_i . betas[d])^2 * (0.5 / sigsqd[d]) over the uploaded rows i (y: FOKL_SLOT_Y,
 * X_i: the columns `slots`, nc of them, as for fokl_predict) and the draws d, reduced over the DRAWS for every row; ll is
 * never stored.  Host memory, row-major: betas [draws, nc], sigsqd [draws] (all positive and finite).
 *   stats_out [rows, 8]     lppd = logsumexp_d(ll) - log(draws); ll_mean; p_waic = the variance of ll over d (divisor
 *                           draws - 1, accumulated about ll[i][0]); and with want_loo (else zeros) elpd_loo, khat, sigma of
 *                           the generalised Pareto fit (0 where khat = +inf), max_d r with r = -ll, and M', the number of
 *                           tail values strictly above the cutoff (M' <= 4, or a tail without a positive lower-quartile
 *                           exceedance: khat = +inf and the raw weights are used)
 *   tail_out  [rows, M + 1] or NULL: the M + 1 largest of r - max r, ascending, M = min(draws / 5, ceil(3 sqrt(draws))); a
 *                           test and diagnostic output (needs want_loo)
 * The estimator is PSIS (Vehtari et al.) with the Zhang-Stephens fit, stated in numpy by score.score_rows_host.  One launch
 * of score_kernel on v_mfma_f64_16x16x4_f64, one wavefront per 16-row tile; merges across lanes in a fixed order, no
 * floating-point atomics: the same arguments give the same bits.
 * Refused (FOKL_ERR_ARG with a text, nothing is launched; the dataset, its slots and pending launches are left alone):
 * a NaN or infinite entry of betas ("every coefficient must be finite"; fokl_score_rows_noise too);
 * want_loo with fewer than FOKL_SCORE_MIN_DRAWS draws or with M + 1 > FOKL_SCORE_MAX_TAIL; basis values and list beyond the
 * LDS of a compute unit; tail_out, coefficient table and statistics together beyond the device's free memory (the message
 * says which is the largest; the environment's FOKL_SCORE_FREE_BYTES, if set, caps what counts as free).
 * Kernel time: FOKL_K_SCORE.  Blocking.
 */
int fokl_score_rows(fokl_ctx *ctx, const int32_t *slots, int nc, const double *betas, const double *sigsqd, int draws,
                    int want_loo, double *stats_out, double *tail_out);

/*
 * The last fokl_score_rows call on `ctx`, out [FOKL_SCORE_REPORT_LEN] (host):
 *   out[0]  the instance (above); zeros after a call that returned an error
 *   out[1]  the grid (workgroups = wavefronts)     out[2]  16-row tiles (more than the grid: the tile loop went round)
 *   out[3]  dynamic LDS bytes     out[4]  tail capacity used, M + 1 (0 without want_loo)
 *   out[5]  rows that took the khat = +inf branch     out[6]  kernel microseconds     out[7]  the noise instance (FOKL_NOISE_*)
 */
int fokl_score_report(const fokl_ctx *ctx, int64_t *out);

/*
 * fokl_score_rows under Student-t noise and / or known row precisions: its arguments, then
 *   nu   INFINITY: Gaussian noise; finite and >= 1: sigsqd[d] is the squared SCALE of t noise with nu degrees of freedom and
 *        ll[i][d] = c_d + log(sw_i) - ((nu + 1) / 2) log1p((sw_i e)^2 / (nu sigsqd[d])), e = y_i - X_i . betas[d],
 *        c_d = log(Gamma((nu + 1) / 2) / Gamma(nu / 2)) - log(nu pi sigsqd[d]) / 2 (the ratio formed as one number)
 *   sw   NULL (ones) or [rows] (host): sqrt of the rows' precisions w_i, finite and > 0; uploaded with the call, its 8 rows
 *        bytes count in the free-memory test.  Gaussian with sw: ll = c_d + log(sw_i) - (sw_i e)^2 (0.5 / sigsqd[d]).
 * Everything after ll is fokl_score_rows' text: new instances of score_kernel, the same tile, merge order and report.
 * nu = INFINITY with sw = NULL is ROUTED to fokl_score_rows (its instance, its bits).  Refused as well: nu NaN or < 1; an sw
 * that is not finite or <= 0.  score.score_rows_host(nu=, sw=) is the statement.
 */
int fokl_score_rows_noise(fokl_ctx *ctx, const int32_t *slots, int nc, const double *betas, const double *sigsqd, int draws,
                          int want_loo, double *stats_out, double *tail_out, double nu, const double *sw);

/* ------------------------------------------------------------------------------------------------------ */
/* The predictive distribution per row: PIT and quantiles (csrc/fokl_predictive_device.inc; fokl_gpy_amd/predictive.py) */
/* ------------------------------------------------------------------------------------------------------ */

/* out[0] of fokl_predictive_report: the instance that ran, a sum of these (0: no call yet, or the last one was refused) */
enum {
    FOKL_PREDICTIVE_NONE = 0,
    FOKL_PREDICTIVE_PIT = 1,        /* with_data: the CDF at the uploaded y from pass 0 */
    FOKL_PREDICTIVE_QUANTILES = 2   /* nq > 0: brackets, first trial and the pass loop */
};
#define FOKL_PREDICTIVE_REPORT_LEN 10
#define FOKL_PREDICTIVE_BASE 6            /* columns of a result row before the quantiles' */
#define FOKL_PREDICTIVE_PER_QUANTILE 5    /* ... and per quantile */
/* Quantiles of one call: a lane keeps q, residual, bracket and two partial sums of each in registers. */
#define FOKL_PREDICTIVE_MAX_QUANTILES 8
/* The largest finite nu of fokl_predictive_rows_noise and the fixed bound of the continued fraction behind the t CDF
 * (csrc/fokl_student.inc; predictive.student_terms is its statement): within the bound every argument has converged for
 * every nu in [1, NU_MAX] (nu = 64 takes 32 iterations at most), and the CDF is within 1e-14 of scipy.special.stdtr there
 * (tests/test_student_host.py).  The CDF itself holds that bound with 64 iterations up to nu = 1 000 (4e-15); the limit stays
 * where the density also agrees with scipy.stats.t.pdf to 1e-14, which it no longer does at nu = 256 (1e-13). */
#define FOKL_PREDICTIVE_NU_MAX 64
#define FOKL_PREDICTIVE_STUDENT_ITERATIONS 40

/*
 * The predictive of row i is the equal-weight mixture over the draws d of N(mu_id, sd[d]^2), mu_id = X_i . betas[d], over
 * the uploaded rows (X_i: the columns `slots`, nc of them, as for fokl_predict; y: FOKL_SLOT_Y, read only with with_data).
 * Host memory, row-major: betas [draws, nc]; sd [draws] = sqrt(sigsqd) and rinv [draws] = 1 / (sd sqrt(2)), positive and
 * finite, formed by the caller; mean_sigsqd = the mean of sigsqd as the caller rounds it; p [nq] strictly inside (0, 1) and
 * distinct, z [nq] their standard normal quantiles (any finite values: only the bracket and the first trial use them);
 * 0 <= nq <= FOKL_PREDICTIVE_MAX_QUANTILES.
 *   out [rows, 6 + 5 nq]    mu_0; s1 = sum_d (mu_d - mu_0); s2 = sum_d (mu_d - mu_0)^2; min_d mu_d; max_d mu_d; pit =
 *                           sum_d 0.5 erfc((mu_d - y) rinv_d) / draws (0 without with_data); then per quantile q, the
 *                           residual r = F(q) - p as last evaluated (+inf: never), the final bracket lo, hi and the passes
 *                           used.  Pass 0 gives lo = min_d (mu_d + sd_d z), hi = max_d (mu_d + sd_d z) and the first trial
 *                           mean + z sqrt(var) (inside the bracket, else its midpoint); each of up to max_passes further
 *                           passes evaluates F and its density at q, moves the bracket and takes a safeguarded Newton step
 *                           or the midpoint, until |r| <= ftol or hi - lo <= xtol (max mu - min mu + max sd).
 * The rule is stated to the last operation in numpy by predictive.predictive_rows_host.  One launch of predictive_kernel on
 * v_mfma_f64_16x16x4_f64, one wavefront per 16-row tile; the product is recomputed in every pass (no limit on the draws);
 * merges across lanes in a fixed order, no atomics: the same arguments give the same bits.
 * Refused (FOKL_ERR_ARG with a text, nothing is launched; the dataset, its slots and pending launches are left alone):
 * a NaN or infinite entry of betas ("every coefficient must be finite"; fokl_predictive_rows_noise too);
 * nq outside its range; p outside (0, 1), not finite or repeated; max_passes < 0; ftol or xtol negative or not finite;
 * neither with_data nor quantiles; basis values beyond the LDS of a compute unit; coefficient table and results together
 * beyond the device's free memory (the environment's FOKL_PREDICTIVE_FREE_BYTES, if set, caps what counts as free).
 * Kernel time: FOKL_K_PREDICTIVE, with the flops of the passes that ran.  Blocking.
 */
int fokl_predictive_rows(fokl_ctx *ctx, const int32_t *slots, int nc, const double *betas, const double *sd, const double *rinv,
                         int draws, double mean_sigsqd, int with_data, const double *p, const double *z, int nq, int max_passes,
                         double ftol, double xtol, double *out);

/*
 * The last fokl_predictive_rows call on `ctx`, out [FOKL_PREDICTIVE_REPORT_LEN] (host):
 *   out[0]  the instance (above); zeros after a call that returned an error
 *   out[1]  the grid (workgroups = wavefronts)     out[2]  16-row tiles (more than the grid: the tile loop went round)
 *   out[3]  dynamic LDS bytes     out[4]  nq
 *   out[5]  the most passes any tile ran (pass 0 not counted)     out[6]  the sum of passes over the tiles
 *   out[7]  unresolved (row, quantile) pairs: |r| > ftol     out[8]  kernel microseconds
 *   out[9]  the noise instance (FOKL_NOISE_*)
 */
int fokl_predictive_report(const fokl_ctx *ctx, int64_t *out);

/*
 * fokl_predictive_rows under Student-t noise and / or known row precisions: its arguments, then
 *   nu   INFINITY: Gaussian components; finite, 1 <= nu <= FOKL_PREDICTIVE_NU_MAX: row i's predictive is the mixture over d
 *        of t_nu(mu_id, scale sd[d] / sw_i); z [nq] are then the quantiles of the standard t_nu (any finite values)
 *   sw   NULL (ones) or [rows] (host): sqrt of the rows' precisions, finite and > 0; uploaded with the call, its 8 rows
 *        bytes count in the free-memory test
 * The passes and the decision rule are fokl_predictive_rows' with k_id = sw_i / sd[d] (Student; Gaussian: rinv[d] sw_i) in
 * the place of rinv[d]: t = (q - mu_d) k_id, F = mean_d T_nu(t), f = mean_d f_nu(t) k_id, pit = mean_d T_nu((y - mu_d) k_id);
 * brackets min / max over d of mu_d + (sd[d] / sw_i) z; first trial mean + z sqrt(var_mu + mean_sigsqd / sw_i^2); width
 * max mu - min mu + max sd / sw_i.  T_nu and f_nu are student_terms (csrc/fokl_student.inc), one continued fraction with
 * the fixed bound above; predictive.predictive_rows_host(nu=, sw=) is the statement.  New instances of predictive_kernel:
 * the same tile, merge order and report; the Student instances take the PIT in a pass of its own (counted in out[5], out[6]).
 * nu = INFINITY with sw = NULL is ROUTED to fokl_predictive_rows (its instance, its bits).  Refused as well: nu NaN or < 1;
 * a finite nu beyond FOKL_PREDICTIVE_NU_MAX; an sw that is not finite or <= 0.
 */
int fokl_predictive_rows_noise(fokl_ctx *ctx, const int32_t *slots, int nc, const double *betas, const double *sd,
                               const double *rinv, int draws, double mean_sigsqd, int with_data, const double *p, const double *z,
                               int nq, int max_passes, double ftol, double xtol, double *out, double nu, const double *sw);

/* ------------------------------------------------------------------------------------------------------ */
/* Which pool rows to measure next: greedy optimal design (csrc/fokl_design_device.inc; fokl_gpy_amd/design.py) */
/* ------------------------------------------------------------------------------------------------------ */

/* out[0] of fokl_design_report: the instance of the three kernels that ran */
enum {
    FOKL_DESIGN_NONE = 0,      /* no call yet, or the last one was refused or failed */
    FOKL_DESIGN_VARIANCE = 1,  /* CMC0 = NULL: greedy D-optimal, v alone */
    FOKL_DESIGN_IVR = 2        /* integrated variance reduction: v and w, the second accumulator chain */
};
#define FOKL_DESIGN_REPORT_LEN 12
/* Columns (ones first) of the pool: a 16-row tile of basis values in LDS is 768 x 16 x 8 B = 96 KiB of the compute unit's
 * 160 KiB, and design_pivot_kernel keeps x*, u and a of that length in its own. */
#define FOKL_DESIGN_MAX_COLUMNS 768

/*
 * Greedy selection of `picks` rows of the uploaded dataset (the pool; X_s: the columns `slots`, nc of them, ones first, as
 * for fokl_predict) given C0 = (G + I / tau^2)^-1 [nc, nc] and, for integrated variance reduction, CMC0 = C0 M C0 [nc, nc]
 * (NULL: greedy D-optimal); both symmetric, host memory, row-major.  With v_s = X_s' C X_s and w_s = X_s' CMC X_s the
 * criterion of a row is v_s, or w_s / (1 + v_s); a pick takes the largest (compared with >: NaN never wins; on equal
 * values the lowest row), and with u = C x*, a = CMC x*, v* = x*' u, w* = x*' a, d = 1 + v*:
 *   C <- C - u u' / d,  CMC <- CMC - (u a' + a u') / d + u u' w* / d^2,
 *   v_s <- v_s - p_s^2 / d,  w_s <- w_s - 2 p_s q_s / d + p_s^2 w* / d^2,   p_s = X_s' u, q_s = X_s' a.
 * Before the first pick, and with refresh_every = r > 0 before the picks r, 2 r, ..., v and w are formed from the current
 * matrices by design_quadform_kernel (v_mfma_f64_16x16x4_f64, one wavefront per 16-row tile) instead of downdated.
 * replicates = 0 masks a picked row.  The statement in numpy is design.select_host.
 *   index_out [picks] int64   the rows in pick order (-1: nothing could be taken, every criterion NaN or -inf)
 *   gain_out  [picks]         the criterion of each pick when it was taken
 *   vstar_out [picks]         v* of each pick (log det A grows by log1p(v*))
 *   x_out     [picks, nc]     the picked rows' columns
 *   v_out, w_out [rows] or NULL: v and w of every row after the last pick's downdate (w_out needs CMC0)
 * All launches (design_quadform_kernel, then design_step_kernel and design_pivot_kernel per pick) are queued on the
 * context's stream and synchronised once; nothing is accumulated with atomics and the best of two rows does not depend on
 * the order they are met in, so the same arguments give the same bits whatever the grid.  grid_cap > 0 caps both grids (a
 * test hook; 0: the device's).
 * Refused (FOKL_ERR_ARG with a text that names the limit, nothing is launched; the dataset, its slots and pending launches
 * are left alone): nc outside 1 .. FOKL_DESIGN_MAX_COLUMNS; picks < 1; picks above the rows without replicates; per-row
 * values and matrices beyond the device's free memory (the environment's FOKL_DESIGN_FREE_BYTES, if set, caps what counts
 * as free).
 * Kernel time: FOKL_K_DESIGN.  Blocking; everything uploaded is freed before it returns.
 */
int fokl_design_select(fokl_ctx *ctx, const int32_t *slots, int nc, const double *C0, const double *CMC0, int picks,
                       int replicates, int refresh_every, int grid_cap, int64_t *index_out, double *gain_out,
                       double *vstar_out, double *x_out, double *v_out, double *w_out);

/*
 * The last fokl_design_select call on `ctx`, out [FOKL_DESIGN_REPORT_LEN] (host):
 *   out[0]  the instance (above); zeros after a call that returned an error
 *   out[1]  the grid of design_quadform_kernel (workgroups = wavefronts)     out[2]  the grid of design_step_kernel
 *   out[3]  16-row tiles (more than out[1]: the tile loop went round)        out[4]  dynamic LDS bytes of a tile
 *   out[5]  picks     out[6]  refreshes (quadratic-form launches after the first)     out[7]  launches in all
 *   out[8]  kernel microseconds of the whole queue     out[9]  ... of the quadratic-form launches
 *   out[10], out[11]  ... of the step and of the pivot launches (measured only while fokl_timing_enable is on, else 0)
 */
int fokl_design_report(const fokl_ctx *ctx, int64_t *out);

/* ------------------------------------------------------------------------------------------------------ */
/* Which pool rows to measure next to find a better optimum: EI and PI over the draws, greedy batch          */
/* (csrc/fokl_acquire_device.inc; fokl_gpy_amd/acquire.py)                                                   */
/* ------------------------------------------------------------------------------------------------------ */

/* `criterion` of fokl_acquire_select and out[0] of fokl_acquire_report: the instance of the kernels that ran */
enum {
    FOKL_ACQUIRE_NONE = 0,     /* no call yet, or the last one was refused or failed */
    FOKL_ACQUIRE_EI = 1,       /* expected improvement: (sum_d max(f_sd - b_d, 0)) / E; a pick sets b_d = max(b_d, f_s*d) */
    FOKL_ACQUIRE_PI = 2        /* probability of improvement: (sum_d [f_sd > b_d]) / E; a pick sets b_d = +inf where f_s*d > b_d */
};
#define FOKL_ACQUIRE_REPORT_LEN 15

/*
 * Greedy selection of `picks` rows of the uploaded dataset (the pool; X_s: the columns `slots`, nc of them, ones first, as
 * for fokl_predict) by expected improvement or probability of improvement over the posterior draws betas [draws, nc]
 * (host, row-major), given the incumbent b [draws] of every draw (finite or -inf).  f_sd = X_s . beta_d is the fitted
 * function, with no noise term; the gain of a row and what a pick does to b are stated at the enum above.  The sense is
 * 'max': a caller that minimises passes -betas and -b (negation is exact).  A pick takes the largest gain among the rows
 * not yet picked (compared with >: NaN never wins; on equal values the lowest row); a row is taken once.  The statement in
 * numpy is acquire.select_host.
 *   lazy != 0: every pick after the first (1) finds the row with the largest gain left from earlier picks
 *   (acquire_bound_kernel), (2) evaluates its 16-row tile fresh, tau = the largest fresh gain among that tile's rows not yet
 *   picked (acquire_pivot_kernel, candidate mode), (3) evaluates only the tiles in which some row not yet picked has an old
 *   gain that is not strictly below tau (acquire_pass_kernel), (4) takes the arg-max (acquire_pivot_kernel, pick mode).
 *   Gains only fall as b rises, exactly so in floating point, so the index and the gain BITS are those of lazy = 0, which
 *   evaluates every tile for every pick (pass, pivot).
 *   index_out     [picks] int64   the rows in pick order (-1: nothing could be taken: every gain NaN)
 *   gain_out      [picks]         the gain of each pick when it was taken (-inf with index -1)
 *   incumbent_out [draws]         b after the last pick ('pi': +inf where the batch improves on the draw)
 *   tiles_out     [picks] int64   16-row tiles evaluated for each pick (lazy = 0: all of them)
 *   trace_pick = k in 0 .. picks - 1 (-1: off): trace_g_out [rows] = the gain of every row as it stood when pick k was taken
 *   (under lazy a skipped tile's rows hold their old gain) and, under lazy, trace_eval_out [tiles] = 1 where the tile was
 *   evaluated for pick k, else 0.  acquire_pass_kernel's own body writes both.
 * Launches: 2 per pick with lazy = 0; 2 for the first pick and 4 for every later one with lazy != 0.  All are queued on
 * the context's stream and synchronised once; nothing is accumulated with atomics and the best of two rows does not
 * depend on the order they are met in, so the same arguments give the same bits whatever the grid.  grid_cap > 0 caps the
 * grids (a test hook; 0: the device's).
 * Refused (FOKL_ERR_ARG with a text that names the limit, nothing is launched; the dataset, its slots and pending launches
 * are left alone): nc < 1, draws < 1, picks < 1, picks above the rows, a coefficient that is not finite, an incumbent that
 * is NaN or +inf, columns whose 16-row tile exceeds 160 KiB of LDS (more than 1280), coefficients and per-row values
 * beyond the device's free memory (the environment's FOKL_ACQUIRE_FREE_BYTES, if set, caps what counts as free).
 * Kernel time: FOKL_K_ACQUIRE.  Blocking; everything uploaded is freed before it returns.
 */
int fokl_acquire_select(fokl_ctx *ctx, const int32_t *slots, int nc, const double *betas, int draws, const double *incumbent,
                        int criterion, int lazy, int picks, int grid_cap, int trace_pick, int64_t *index_out, double *gain_out,
                        double *incumbent_out, int64_t *tiles_out, double *trace_g_out, unsigned char *trace_eval_out);

/*
 * The last fokl_acquire_select call on `ctx`, out [FOKL_ACQUIRE_REPORT_LEN] (host):
 *   out[0]  the instance (above); zeros after a call that returned an error     out[1]  lazy (1) or not (0)
 *   out[2]  the grid of acquire_pass_kernel (workgroups = wavefronts)           out[3]  the grid of acquire_bound_kernel
 *   out[4]  16-row tiles     out[5]  dynamic LDS bytes of a tile     out[6]  16-draw tiles per block of the product (DT)
 *   out[7]  picks     out[8]  launches in all     out[9]  tiles evaluated in total
 *   out[10] tiles evaluated by the most expensive pick after the first under lazy (0 without lazy or with one pick)
 *   out[11] kernel microseconds of the whole queue
 *   out[12], out[13], out[14]  ... of the pass, bound and pivot launches (measured only while fokl_timing_enable is on, else 0)
 */
int fokl_acquire_report(const fokl_ctx *ctx, int64_t *out);

/* ------------------------------------------------------------------------------------------------------ */
/* The same selection under limits on other models' outputs (csrc/fokl_acquire_system_device.inc;            */
/* fokl_gpy_amd/acquire.py: acquire_system)                                                                  */
/* ------------------------------------------------------------------------------------------------------ */

#define FOKL_ACQUIRE_SYSTEM_MAX_MODELS 8       /* the objective and up to 7 constraint models */
#define FOKL_ACQUIRE_SYSTEM_INCUMBENT 3        /* out[0] of the report after the incumbent call (1, 2: the criterion of a selection) */
#define FOKL_ACQUIRE_SYSTEM_REPORT_LEN 16

/*
 * The greedy selection above with feasibility per (row, draw).  Model 0 is the objective, models 1 .. n_constraints
 * (1 to 7) are constraint models; draw d is row d of every model's coefficients.
 *   widths [n_constraints + 1]   the columns nc_k of every model (>= 1)
 *   slots  [sum nc_k]            the models' column slots one model behind the other (ones first in each, as for fokl_predict)
 *   betas                        the models' coefficients one model behind the other, [draws, nc_k] row-major each (host)
 *   lo, hi [n_constraints]       the limits of constraint model k + 1; either may be infinite, neither NaN
 * With f_sd = X0_s . beta0_d and g_ksd = Xk_s . betak_d, a draw is feasible at a row when every k has lo <= g_ksd <= hi (a
 * NaN g is infeasible).  The gain of a row is the sum over its FEASIBLE draws of fokl_acquire_select's terms, over `draws`;
 * an infeasible draw contributes exactly 0.0 whatever f is, and a pick changes b in its feasible draws only.  Everything
 * else -- the arg-max, ties, NaN, lazy, the traces, the launches per pick, grid_cap -- is fokl_acquire_select's, and with
 * infinite limits every output is its output, bit for bit.  The statement in numpy is acquire.select_system_host.
 *   feasible_out [picks] int64   the draws in which each picked row is feasible (0 with index -1)
 * A 16-row tile holds every model's basis values, each model padded to a multiple of 4 columns on its own.
 * Refused (FOKL_ERR_ARG with a text that names the limit, nothing is launched): what fokl_acquire_select refuses,
 * n_constraints outside 1 .. 7, a width below 1, a NaN limit, padded columns of all models beyond 1280 (160 KiB of LDS),
 * the memory rule with FOKL_ACQUIRE_FREE_BYTES.  Kernel time: FOKL_K_ACQUIRE_SYSTEM.  Blocking; everything uploaded is freed
 * before it returns.
 */
int fokl_acquire_system_select(fokl_ctx *ctx, const int32_t *slots, const int32_t *widths, int n_constraints, const double *betas,
                               int draws, const double *incumbent, const double *lo, const double *hi, int criterion, int lazy,
                               int picks, int grid_cap, int trace_pick, int64_t *index_out, double *gain_out,
                               double *incumbent_out, int64_t *tiles_out, int64_t *feasible_out, double *trace_g_out,
                               unsigned char *trace_eval_out);

/*
 * Over the uploaded rows (the measured points), per draw: best_out [draws] = the largest f over the rows feasible in that
 * draw, -inf if there is none, NaN if a feasible row's f is not finite; count_out [draws] int64 = the feasible rows.
 * Arguments and refusals as above.  One wavefront per 16-row tile keeps its workgroup's result per draw, a second kernel
 * merges the workgroups in index order: no atomics, and the same arguments give the same bits whatever the grid (grid_cap
 * > 0 caps it; a test hook).  The statement in numpy is acquire.incumbent_system_host.  Kernel time:
 * FOKL_K_ACQUIRE_SYSTEM.  Blocking.
 */
int fokl_acquire_system_incumbent(fokl_ctx *ctx, const int32_t *slots, const int32_t *widths, int n_constraints,
                                  const double *betas, int draws, const double *lo, const double *hi, int grid_cap,
                                  double *best_out, int64_t *count_out);

/*
 * The last fokl_acquire_system_select or fokl_acquire_system_incumbent call on `ctx`, out [FOKL_ACQUIRE_SYSTEM_REPORT_LEN]:
 *   out[0]  the instance: FOKL_ACQUIRE_EI / FOKL_ACQUIRE_PI of a selection, FOKL_ACQUIRE_SYSTEM_INCUMBENT; zeros after a
 *           call that returned an error            out[1]  lazy (1) or not (0)       out[2]  constraint models (K)
 *   out[3]  the grid of the pass kernel (of the incumbent kernel)     out[4]  the grid of acquire_bound_kernel (of the merge)
 *   out[5]  16-row tiles     out[6]  dynamic LDS bytes of a tile     out[7]  draws per block of the product: the draw group (64)
 *   out[8]  picks     out[9]  launches in all     out[10] tiles evaluated in total
 *   out[11] tiles evaluated by the most expensive pick after the first under lazy (0 without lazy or with one pick)
 *   out[12] kernel microseconds of the whole queue
 *   out[13], out[14], out[15]  ... of the pass, bound and pivot launches (a selection: measured only while
 *           fokl_timing_enable is on, else 0; the incumbent call: its two kernels in out[13] and out[14])
 */
int fokl_acquire_system_report(const fokl_ctx *ctx, int64_t *out);

/* ------------------------------------------------------------------------------------------------------ */
/* Every draw's best rows of a pool, ranked (csrc/fokl_drawbest_device.inc; fokl_gpy_amd/pooloptimum.py)     */
/* ------------------------------------------------------------------------------------------------------ */

#define FOKL_DRAWBEST_MAX_RANKS 64
#define FOKL_DRAWBEST_MAX_COLUMNS 1280         /* a 16-row tile of basis values in LDS: 160 KiB */
#define FOKL_DRAWBEST_REPORT_LEN 14

/*
 * Over the uploaded rows (the pool), f_sd = sum_k column(slots[k])[s] * betas[d][k], sense 'max'.  The candidates of draw
 * d are the rows with mask[s] == 0 (mask NULL: all) whose f_sd is not NaN; +inf and -inf compare as numbers.  The order is
 * value descending, on equal values row ascending.  index_out [ranks][draws] int64, value_out [ranks][draws]: the r-th
 * candidate of draw d in that order and its f; a draw with fewer than r + 1 candidates has index -1 and value -inf from
 * there on.  f is never stored.  The statement in numpy is pooloptimum.ranks_host: on integer data both outputs are its
 * bits; on continuous data the sums run in another order and a row may differ where two values tie to rounding.
 * Host memory, row-major: slots [nc], betas [draws, nc] finite, mask [rows] or NULL.
 * Rank r is one launch of drawbest_kernel over row chunks x blocks of 128 draws (rank r > 0: only what lies strictly after
 * rank r - 1 of the draw, read on the device) and one of drawbest_merge_kernel over the chunks' records: 2 * ranks launches
 * on the context's stream with no host wait between them.  No atomics; the same arguments give the same bits whatever the
 * grid (grid_cap > 0 caps the row chunks; a test hook).
 * Refused (FOKL_ERR_ARG with a text that names the limit, nothing is launched): more than FOKL_DRAWBEST_MAX_COLUMNS
 * columns, ranks outside 1..FOKL_DRAWBEST_MAX_RANKS, a coefficient that is not finite, a call whose buffers and 64 MiB to
 * spare reach beyond the device's free memory (the environment's FOKL_ACQUIRE_FREE_BYTES, if set, caps what counts as
 * free).  Kernel time: FOKL_K_DRAWBEST (the whole queue).  Blocking; everything uploaded is freed before it returns.
 */
int fokl_drawbest_rows(fokl_ctx *ctx, const int32_t *slots, int nc, const double *betas, int draws,
                       const unsigned char *mask, int ranks, int grid_cap, int64_t *index_out, double *value_out);

/*
 * The last fokl_drawbest_rows call on `ctx`, out [FOKL_DRAWBEST_REPORT_LEN] (host):
 *   out[0]  the instance: 0 none (no call yet, or the last one was refused or failed: all zeros), 1 ran     out[1]  ranks
 *   out[2]  16-row tiles     out[3]  row chunks     out[4]  draw blocks (128 draws)
 *   out[5]  the grid of drawbest_kernel: row chunks, rounded up to 8, x draw blocks     out[6]  the grid of the merge
 *   out[7]  dynamic LDS bytes     out[8]  where the coefficients lived (FOKL_POPULATION_REGISTERS: at most 128 columns, padded
 *           to 4; FOKL_POPULATION_TABLE)     out[9]  launches in all     out[10] 16-row tiles per chunk
 *   out[11] kernel microseconds of the whole queue
 *   out[12], out[13]  ... of the passes and of the merges (measured only while fokl_timing_enable is on, else 0)
 */
int fokl_drawbest_report(const fokl_ctx *ctx, int64_t *out);

/* ------------------------------------------------------------------------------------------------------ */
/* Unknown inputs from observed outputs (csrc/fokl_infer_device.inc; fokl_gpy_amd/infer.py)                  */
/* ------------------------------------------------------------------------------------------------------ */

/* out[0] of fokl_infer_report: the lane mapping that ran */
enum {
    FOKL_INFER_NONE = 0,            /* no call yet, or the last one was refused or failed */
    FOKL_INFER_WALKER_PER_LANE = 1  /* one draw per wavefront, lane = walker; the half that does not move idles */
};
#define FOKL_INFER_REPORT_LEN 9
#define FOKL_INFER_WALKERS 64
/* Term evaluations by a wavefront (one term of the model at one observation, for its 64 lanes) asked of ONE launch:
 * the draws are sliced over launches so that draws x (2 (burnin + draws) + 1) x K x max(n_terms, 1) stays below it (a
 * slice holds at least one draw).  At the roughly 40 ns a wavefront needs per term evaluation and with every SIMD of
 * the part holding one ensemble, 2^33 is some hundreds of milliseconds of a full device: far below any watchdog, and
 * long enough that the launch overhead is nothing.  `term_cap` of fokl_infer_inputs replaces it (a test hook). */
#define FOKL_INFER_TERM_CAP ((int64_t)1 << 33)

/*
 * For every posterior draw e an ensemble of 64 walkers samples the d unknown inputs theta (normalised coordinates) from
 *   lp_e(theta) = -h[e] sum_k (y[k] - f_ek(theta))^2 - 1/2 sum_i prior_prec[i] (theta_i - prior_mean[i])^2   inside lo < theta < hi,
 *   f_ek(theta) = sum_t (betas[e][t] known_prod[k][t]) U_t(theta),  t = 0 .. n_terms ascending, U_0 = 1,
 * U_t the product of term t's factors in the unknown inputs (row t - 1 of mtx_u, ascending input order), each factor by
 * Horner from `table`.  The sampler -- stretch moves, a differential-evolution jump every `jump_every`-th iteration (0:
 * never), half 0 of the walkers then half 1, a proposal outside the box rejected without an evaluation -- is stated in numpy
 * by infer.sample_host (the module docstring is the statement).  Random numbers: Philox 4x32-10 keyed by (seed, draw_ids[e]
 * or e), counter (iteration, purpose, index, 1) -- fokl_infer_rng below.
 * Host memory, row-major:
 *   mtx_u [n_terms, d] int32, betas [n_draws, n_terms + 1], h [n_draws] (0.5 / sigma^2: positive, finite), draw_ids
 *   [n_draws] or NULL, table [n_basis, width] as for fokl_model_optimize, lo / hi / prior_mean / prior_prec [d],
 *   y [K], known_prod [K, n_terms + 1], starts [64, d] strictly inside the box
 *   x_out  [n_draws, kept, 64, d], lp_out [n_draws, kept, 64]   kept = ceil(draws / thin); row r is the state after both halves
 *          of iteration burnin + r thin.  Both NULL: no rows are kept
 *   sums_out [n_draws, 64, 2, 2, d]   per walker and half of the post-burn-in iterations (the first draws / 2, the rest): the
 *          sum and the sum of squares of theta_i - (lo_i + hi_i) / 2, in iteration order
 *   accept_out [n_draws, 64, 2] int32  accepted stretch moves, accepted jump moves (burn-in included)
 *   evals_out [n_draws] int64          evaluations of the target (the 64 of the starts included)
 * One wavefront per workgroup and draw, lane = walker; positions, proposals and factor values in LDS as [item][lane], a
 * partner's position an LDS read at a computed lane; the draw's coefficients, premultiplied by known_prod on the host,
 * are scalar loads.  The model is evaluated by fokl_optimize_core.inc's op_factors / op_terms.  No atomics: the same
 * arguments give the same bits, and neither draw_ids' order, thin nor the slicing into launches (`term_cap`; 0:
 * FOKL_INFER_TERM_CAP) changes a bit of a draw's chain.
 * Refused (FOKL_ERR_ARG with a text that names the limit, nothing is launched; the dataset, its slots and pending launches
 * are left alone): d outside 1 .. 16; lo >= hi or not finite; a start not strictly inside the box; h not positive and
 * finite; K < 1; an order beyond the table; more than 288 values per lane in LDS (3 per distinct (input, order) factor +
 * 4 d); thin < 1, draws < 1, burnin < 0, jump_every < 0; a negative or non-finite prior precision; NaN or infinity in
 * betas x known_prod, y or the prior mean; outputs and coefficients beyond the device's free memory (the environment's
 * FOKL_INFER_FREE_BYTES, if set, caps what counts as free).
 * Kernel time: FOKL_K_INFER.  Blocking; everything uploaded is freed before it returns.
 */
int fokl_infer_inputs(fokl_ctx *ctx, int d, int n_terms, const int32_t *mtx_u, int n_draws, const double *betas,
                      const double *h, const uint32_t *draw_ids, const double *table, int n_basis, int width,
                      const double *lo, const double *hi, const double *prior_mean, const double *prior_prec, int K,
                      const double *y, const double *known_prod, const double *starts, int burnin, int draws, int thin,
                      int jump_every, uint32_t seed, int64_t term_cap, double *x_out, double *lp_out, double *sums_out,
                      int32_t *accept_out, int64_t *evals_out);

/*
 * The last fokl_infer_inputs call on `ctx`, out [FOKL_INFER_REPORT_LEN] (host):
 *   out[0]  the lane mapping (above); zeros after a call that returned an error
 *   out[1]  LDS values per lane     out[2]  the grid of the largest launch (workgroups = wavefronts = draws)
 *   out[3]  launches     out[4]  kernel microseconds over all launches     out[5]  iterations of a chain (burnin + draws)
 *   out[6]  target evaluations over all draws     out[7]  draws per launch     out[8]  dynamic LDS bytes
 */
int fokl_infer_report(const fokl_ctx *ctx, int64_t *out);

/*
 * out[j], j < count: the number the sampler draws for `purpose` and index j at `iteration` of posterior draw `draw_id`:
 * purposes 0, 1, 2 the uniforms u1, u2, u3 of walker j in [0, 1), 3 the jump move's normal of index 64 i + w.  Host code,
 * no device.  FOKL_ERR_ARG for another purpose.
 */
int fokl_infer_rng(uint32_t seed, uint32_t draw_id, uint32_t iteration, int purpose, int count, double *out);

/* ------------------------------------------------------------------------------------------------------ */
/* What the last fokl_gp_integrate_ensemble (fokl_hip.h; csrc/fokl_integrate_device.inc) ran                */
/* ------------------------------------------------------------------------------------------------------ */

#define FOKL_INTEGRATE_REPORT_LEN 10

/*
 * The last fokl_gp_integrate_ensemble call on `ctx`, out [FOKL_INTEGRATE_REPORT_LEN] (host values, no launch); zeros after a
 * call that was refused or failed:
 *   out[0]  NS: the kernel instance (states)     out[1]  members     out[2]  workgroups = wavefronts = ceil(members / 64)
 *   out[3]  the integration kernel's dynamic LDS bytes     out[4]  integration launches     out[5]  steps per launch
 *   out[6]  the band kernel's dynamic LDS bytes: its sorted list, 0 without bounds
 *   out[7]  (state, point) rows of the first launch, the largest     out[8]  workgroups of the band kernel in that launch
 *   (fewer than the rows: a workgroup goes round the grid)     out[9]  compute units of the device
 */
int fokl_gp_integrate_report(const fokl_ctx *ctx, int64_t *out);

/* ------------------------------------------------------------------------------------------------------ */
/* A system of fitted models over every posterior draw (csrc/fokl_simulate_device.inc; fokl_gpy_amd/dynamics.py) */
/* ------------------------------------------------------------------------------------------------------ */

#define FOKL_SIMULATE_REPORT_LEN 8
#define FOKL_SIMULATE_MAX_STATES 8

/*
 * A system of fitted models as dynamics._prepare assembles it: what fokl_simulate_ensemble, fokl_simulate_adaptive,
 * fokl_simulate_stiff, fokl_steady_states, fokl_assimilate_ensemble, fokl_calibrate_ensemble, fokl_control_solve,
 * fokl_control_pooled_solve and fokl_control_cvar_solve integrate (fokl_steady_states: bring to rest).  Host memory, row-major;
 * the call reads it and keeps no pointer.
 */
typedef struct fokl_system {
    int n_members;          /* members = posterior draws / initial states (the control and filter calls: n_draws) */
    int n_states;           /* d(state k)/dt = model_k(its inputs), k < n_states <= FOKL_SIMULATE_MAX_STATES */
    int64_t n_steps;        /* steps of size h; the time axis has n_steps + 1 points */
    double h;
    int n_forcing_cols;
    const double *forcing;  /* [n_steps, n_forcing_cols] true scale; row s serves every stage of step s */
    /* the normalised inputs v = (x - lo) / span clamped to [0, 1]: the first n_norm_forcing read forcing column
     * -(src + 1), the others state src, in ascending order of src */
    int n_norm_forcing, n_norm;
    const int32_t *norm_src; /* [n_norm] */
    const double *norm_lo, *norm_span;
    /* the distinct factors, the first n_forcing_factors on forcing inputs, inside either group kind 0 (cubic splines)
     * before kind 1 (Bernoulli); fac_row is the factor's row of its table, fac_degree a Bernoulli factor's order (<= 20) */
    int n_forcing_factors, n_factors;
    const int32_t *fac_norm, *fac_kind, *fac_row, *fac_degree; /* [n_factors] */
    int n_spline_rows;
    const double *spline_table; /* [n_spline_rows, 499, 4]: c0 .. c3 of every piece */
    int n_bern_rows;
    const double *bern_table; /* [n_bern_rows, 21], lowest power first */
    /* entries [n_entries][4] int32 {slot, slot, slot, coefficient}: slot 0 is 1.0, slot f + 1 factor f; coefficient -1:
     * the product continues in the next entry.  Model k owns entries [entry_begin[k], entry_begin[k] + entry_count[k])
     * and its constant is coefficient constant[k] */
    int n_entries;
    const int32_t *entries, *entry_begin, *entry_count, *constant;
    int n_coef;
    /* The one layout that differs between the calls: the simulate calls take coef as [n_coef][n_members] (a coefficient's
     * members are contiguous), the assimilate, calibrate and control calls as [n_draws][n_coef] (a draw's coefficients are) */
    const double *coef;
    const double *y0;  /* [n_states, n_members] */
    const double *box; /* [n_states, 2] true scale: lower < upper */
} fokl_system;

/*
 * Classical Runge-Kutta integration of `system` for all its members at once.  The arithmetic is stated by
 * dynamics.simulate_host (the module docstring of fokl_gpy_amd/dynamics.py): a member's trajectory equals the host
 * statement's bit for bit.  coef [n_coef, n_members].  Host memory, row-major:
 *   mean [n_states, n_steps + 1]; bounds [n_states, n_steps + 1, 2] or NULL (sorted[cut], sorted[n_members - cut], at most
 *   16 384 members); members [n_members, n_states, n_steps + 1] or NULL; first_saturation [n_members] int32: the first step
 *   in which a clamp or the slope rule acted, -1 never.
 * One lane per member, one wavefront per workgroup, (1 + n_factors + n_norm - n_norm_forcing + n_coef) values per lane in
 * LDS (at most 144 KB).  The steps are cut into launches of FOKL_SIMULATE_STEPS_PER_LAUNCH (environment, default 512): the
 * cut changes no bit.  Refused (FOKL_ERR_ARG with a text that names the limit, nothing is launched, the dataset and
 * pending launches are left alone): a NULL system, more than 8 states, an index outside its table, an empty box, the LDS
 * budget, bounds over fewer than 2 or more than 16 384 members.  Kernel times: FOKL_K_INTEGRATE, FOKL_K_BAND.  Blocking.
 */
int fokl_simulate_ensemble(fokl_ctx *ctx, const fokl_system *system, int cut, double *mean, double *bounds, double *members,
                           int32_t *first_saturation);

/*
 * The last fokl_simulate_ensemble call on `ctx`, out [FOKL_SIMULATE_REPORT_LEN] (host values, no launch); zeros after a call
 * that was refused or failed:
 *   out[0]  NS: the kernel instance (states)     out[1]  members     out[2]  workgroups = wavefronts = ceil(members / 64)
 *   out[3]  dynamic LDS bytes     out[4]  integration launches     out[5]  spline factors     out[6]  Bernoulli factors
 *   out[7]  steps per launch
 */
int fokl_simulate_report(const fokl_ctx *ctx, int64_t *out);

/* ------------------------------------------------------------------------------------------------------ */
/* The same system integrated under an error tolerance (csrc/fokl_simulate_adaptive_device.inc; dynamics.py) */
/* ------------------------------------------------------------------------------------------------------ */

#define FOKL_SIMULATE_ADAPTIVE_REPORT_LEN 12
#define FOKL_SIMULATE_ADAPTIVE_MAX_HALVINGS 12

/*
 * fokl_simulate_ensemble's system, plan and Runge-Kutta step on the same output grid, every member choosing its own substeps
 * inside each output step by step doubling on a dyadic grid: at level k a trial is one step of 2 g and two steps of
 * g = h / 2^(k + 1), accepted where |y2 - y1| <= 15 (atol_j + rtol max(|y_j|, |y2_j|)) for every state j or k == max_halvings.
 * The arithmetic is stated by dynamics.simulate_adaptive_host (the module docstring of fokl_gpy_amd/dynamics.py): every
 * output equals the host statement's bit for bit.  `system` and `cut` are fokl_simulate_ensemble's; then
 *   rtol, atol [n_states]; min_halvings <= max_halvings: the levels a member may use
 *   mean, bounds, members, first_saturation: as fokl_simulate_ensemble's
 *   pairs, rejected [n_members] int64: accepted pairs of half steps, rejected trials
 *   max_level [n_members] int32: the deepest level of an accepted pair; error [n_members]: the largest accepted
 *   |y2 - y1| / (15 sc); first_unresolved [n_members] int32: the first step in which a pair was accepted at max_halvings
 *   outside the tolerance, -1 never; levels [n_members, n_steps] int8 or NULL: the deepest level accepted inside each step.
 * One lane per member, one wavefront per workgroup, fokl_simulate_ensemble's LDS layout and bound; a lane that has finished
 * an output step waits for the slowest lane of its wavefront.  The steps are cut into launches of
 * max(1, FOKL_SIMULATE_ADAPTIVE_PAIRS_PER_LAUNCH >> max_halvings) steps (environment, default 65 536): the cut changes no bit.
 * No atomics: member e of a large run equals member e run alone.  Refused (FOKL_ERR_ARG with a text that names the limit,
 * nothing is launched): what fokl_simulate_ensemble refuses, rtol or an atol that is negative or not finite, rtol == 0 with
 * a zero atol, levels outside 0 <= min_halvings <= max_halvings <= 12.  Kernel times: FOKL_K_INTEGRATE, FOKL_K_BAND.  Blocking.
 */
int fokl_simulate_adaptive(fokl_ctx *ctx, const fokl_system *system, int cut, double rtol, const double *atol,
                           int min_halvings, int max_halvings, double *mean, double *bounds, double *members,
                           int32_t *first_saturation, int64_t *pairs, int64_t *rejected, int32_t *max_level, double *error,
                           int32_t *first_unresolved, int8_t *levels);

/*
 * The last fokl_simulate_adaptive call on `ctx`, out [FOKL_SIMULATE_ADAPTIVE_REPORT_LEN] (host values, no launch); zeros
 * after a call that was refused or failed:
 *   out[0]  NS: the kernel instance (states)     out[1]  members     out[2]  workgroups = wavefronts = ceil(members / 64)
 *   out[3]  integration launches     out[4]  steps per launch     out[5]  dynamic LDS bytes     out[6]  spline factors
 *   out[7]  Bernoulli factors     out[8]  min_halvings     out[9]  max_halvings     out[10] accepted pairs, all members
 *   out[11] rejected trials, all members
 */
int fokl_simulate_adaptive_report(const fokl_ctx *ctx, int64_t *out);

/* ------------------------------------------------------------------------------------------------------ */
/* The same system for stiff members: Rodas3 (csrc/fokl_simulate_stiff_device.inc; dynamics.py)             */
/* ------------------------------------------------------------------------------------------------------ */

#define FOKL_SIMULATE_STIFF_REPORT_LEN 11

/*
 * fokl_simulate_adaptive's system, plan, output grid and per-member dyadic step control with a linearly implicit step: at
 * level k a trial is one Rodas3 step of g = h / 2^k (four stages, order 3 with an embedded order 2, gamma = 1 / 2, L-stable):
 * the Jacobian of the right-hand side by forward tangents, W = (2 / g) I - J factorised once by LU with partial pivoting,
 * four solves; accepted where the estimate |K4_j| <= atol_j + rtol max(|y_j|, |y_new_j|) for every state j or
 * k == max_halvings.  The arithmetic is stated by dynamics.simulate_stiff_host (the module docstring of
 * fokl_gpy_amd/dynamics.py): every output equals the host statement's bit for bit.  The arguments are
 * fokl_simulate_adaptive's, except
 *   steps, rejected, swaps [n_members] int64: accepted steps, rejected trials, row exchanges in the factorisations of the
 *   accepted steps; error [n_members]: the largest accepted |K4| / sc.
 * One lane per member, one wavefront per workgroup; W, the pivot rows and the stages are per-lane registers; LDS holds
 * fokl_simulate_ensemble's rows and one set of tangent rows: (2 (1 + factors + normalised states) + coefficients) x 64 x 8
 * bytes.  The steps are cut into launches of max(1, FOKL_SIMULATE_STIFF_SUBSTEPS_PER_LAUNCH >> max_halvings) output steps
 * (environment, default 65 536): the cut changes no bit.  No atomics: member e of a large run equals member e run alone.
 * Refused (FOKL_ERR_ARG with a text that names the limit, nothing is launched): what fokl_simulate_adaptive refuses, and a
 * system whose LDS need exceeds the 144 KB of a wavefront.  Kernel times: FOKL_K_INTEGRATE, FOKL_K_BAND.  Blocking.
 */
int fokl_simulate_stiff(fokl_ctx *ctx, const fokl_system *system, int cut, double rtol, const double *atol, int min_halvings,
                        int max_halvings, double *mean, double *bounds, double *members, int32_t *first_saturation,
                        int64_t *steps, int64_t *rejected, int64_t *swaps, int32_t *max_level, double *error,
                        int32_t *first_unresolved, int8_t *levels);

/*
 * The last fokl_simulate_stiff call on `ctx`, out [FOKL_SIMULATE_STIFF_REPORT_LEN] (host values, no launch); zeros after a
 * call that was refused or failed:
 *   out[0]  NS: the kernel instance (states)     out[1]  members     out[2]  workgroups = wavefronts = ceil(members / 64)
 *   out[3]  integration launches     out[4]  output steps per launch     out[5]  dynamic LDS bytes     out[6]  min_halvings
 *   out[7]  max_halvings     out[8]  accepted steps, all members     out[9]  rejected trials, all members
 *   out[10] row exchanges of the accepted steps, all members
 */
int fokl_simulate_stiff_report(const fokl_ctx *ctx, int64_t *out);

/* ------------------------------------------------------------------------------------------------------ */
/* Where the same system comes to rest: steady states (csrc/fokl_steady_device.inc; dynamics.py)             */
/* ------------------------------------------------------------------------------------------------------ */

#define FOKL_STEADY_REPORT_LEN 8
#define FOKL_STEADY_MAX_ITER 200
#define FOKL_STEADY_MAX_HALVINGS 30

/*
 * A damped Newton iteration on F(y) = 0 for every (operating point, member), F and its Jacobian J being fokl_simulate_stiff's
 * stage with a step of 1 (clamps and slope rule included): W = -J with 1 on the diagonal of a held row (F_k == 0 and row k of
 * J zero), delta = W^-1 F by the same LU, and the first of y + delta 2^-b, b = 0 .. max_halvings, clipped to the box, that
 * lowers r = max_j |F_j| / ftol_j.  The arithmetic is stated by dynamics.steady_states_host (the module docstring of
 * fokl_gpy_amd/dynamics.py): every output equals the host statement's bit for bit.  In `system` n_steps = Q is the number of
 * operating points and row q of forcing is point q; n_members = draws x starts, member e S + s being draw e from start s, so
 * coef [n_coef, n_members] repeats a draw's coefficients per start and y0 [n_states, n_members] holds the starts; h is not
 * used.  Host memory, row-major:
 *   ftol [n_states]; max_iter in 1 .. 200; max_halvings in 0 .. 30
 *   y [Q, n_members, n_states]: the final state; residual [Q, n_members]: the final r; iterations, halvings [Q, n_members]
 *   int32 (halvings: the trial points refused, all iterations); status [Q, n_members] int8: 0 converged (r <= 1), 1 the
 *   iteration limit, 2 stalled (no trial point lowered r), 3 r not finite; on_wall [Q, n_members, n_states] uint8: the state
 *   was held at the last evaluation; jacobian [Q, n_members, n_states, n_states] or NULL: J at the final state.
 * One lane per member, one wavefront per workgroup and operating point, fokl_simulate_stiff's LDS rows and bound; both loops
 * have the bounds above, and a lane that has ended waits for the slowest lane of its wavefront.  The points are cut into
 * launches of at most FOKL_STEADY_POINTS_PER_LAUNCH (environment, default 4 096): the cut changes no bit.  No atomics: a
 * member of a large run equals that member run alone.  Refused (FOKL_ERR_ARG with a text that names the limit, nothing is
 * launched): what fokl_simulate_stiff refuses of a system, the LDS budget included, no operating point, max_iter or
 * max_halvings outside their ranges, an ftol that is not positive and finite.  Kernel time: FOKL_K_INTEGRATE.  Blocking.
 */
int fokl_steady_states(fokl_ctx *ctx, const fokl_system *system, const double *ftol, int max_iter, int max_halvings, double *y,
                       double *residual, int32_t *iterations, int8_t *status, int32_t *halvings, uint8_t *on_wall,
                       double *jacobian);

/*
 * The last fokl_steady_states call on `ctx`, out [FOKL_STEADY_REPORT_LEN] (host values, no launch); zeros after a call that
 * was refused or failed:
 *   out[0]  NS: the kernel instance (states)     out[1]  members     out[2]  workgroups = ceil(members / 64) x points
 *   out[3]  dynamic LDS bytes     out[4]  launches     out[5]  operating points     out[6]  iterations, all members
 *   out[7]  halvings, all members
 */
int fokl_steady_report(const fokl_ctx *ctx, int64_t *out);

/* ------------------------------------------------------------------------------------------------------ */
/* A particle filter of such a system against measurements (csrc/fokl_assimilate_device.inc; dynamics.py)    */
/* ------------------------------------------------------------------------------------------------------ */

#define FOKL_ASSIMILATE_REPORT_LEN 9
#define FOKL_ASSIMILATE_PARTICLES 64

/*
 * A bootstrap particle filter per posterior draw: 64 particles follow fokl_simulate_ensemble's Runge-Kutta step with the
 * draw's coefficients, receive process noise, and are weighted and resampled at the observed points.  The plan of the system
 * is dynamics._prepare's (`system`, with coef by draw), the
 * arithmetic is stated by dynamics.assimilate_host (the module docstring of fokl_gpy_amd/dynamics.py).  Host memory,
 * row-major:
 *   coef [n_draws, n_coef] with n_draws = system->n_members; draw_ids [n_draws]: the second key word of a draw's random
 *          numbers (fokl_assimilate_rng)
 *   obs_state [n_observed] the state every measured column reads (distinct), obs_sd [n_observed] > 0
 *   obs_row [n_steps + 1] int32: the row of `data` measured at a point, -1 none; the rows appear as 0, 1, ... n_obs - 1
 *   data [n_obs, n_observed] true scale, NaN = missing; obs_const [n_obs] = the sum over a row's present entries of
 *          log(obs_sd sqrt(2 pi)), subtracted from the row's evidence increment
 *   process_q [n_states] = process_sd sqrt(h) >= 0 (0: no number is drawn), y0_sd [n_states] >= 0
 *   threshold = resample_below x 64 in [0, 64]: a row resamples where its ESS is below it
 *   stats [n_draws, n_obs, 2 n_states + 3]: the weighted means of the states, their weighted variances, the ESS (all
 *          before resampling), the increment of the log evidence (-inf: the draw collapsed here), 1.0 if it resampled
 *   particles_out [n_draws, n_obs, 64, n_states] and weights_out [n_draws, n_obs, 64], before resampling; both or neither NULL
 *   first_saturation [n_draws] int32: the first step in which a clamp or the slope rule acted for any particle, -1 never
 *   collapsed [n_draws] int32: the first row at which no particle had a positive weight, -1 never
 * One wavefront per workgroup and draw, lane = particle; LDS bytes = (1 + n_factors + n_norm - n_norm_forcing) x 64 x 8 +
 * 64 x 8 (the exchange row) + n_coef x 8, at most 144 KB -- the coefficients are held once, so systems that
 * fokl_simulate_ensemble refuses for LDS run here.  Sums and maxima over the particles are xor butterflies (offsets 32 .. 1),
 * the prefix sum a Hillis-Steele scan (offsets 1 .. 32); no atomics: the same arguments give the same bits.  The steps are
 * cut into launches of FOKL_ASSIMILATE_STEPS_PER_LAUNCH (environment, default 512): the cut changes no bit.
 * Refused (FOKL_ERR_ARG with a text that names the limit, nothing is launched, the dataset and pending launches are left
 * alone): what fokl_simulate_ensemble refuses of a system (its LDS bound excepted), the LDS bytes above, an observed column
 * outside the states or twice the same, obs_sd not positive, negative noise, a threshold outside [0, 64], no observation,
 * an observation table that is not 0, 1, ... in order or disagrees with n_obs.
 * Kernel time: FOKL_K_INTEGRATE.  Blocking; everything uploaded is freed before it returns.
 */
int fokl_assimilate_ensemble(fokl_ctx *ctx, const fokl_system *system, const uint32_t *draw_ids, int n_observed,
                             const int32_t *obs_state, const double *obs_sd, int n_obs, const int32_t *obs_row,
                             const double *data, const double *obs_const, const double *process_q, const double *y0_sd,
                             double threshold, uint32_t seed, double *stats, double *particles_out, double *weights_out,
                             int32_t *first_saturation, int32_t *collapsed);

/*
 * The last fokl_assimilate_ensemble call on `ctx`, out [FOKL_ASSIMILATE_REPORT_LEN] (host values, no launch); zeros after a
 * call that was refused or failed:
 *   out[0]  NS: the kernel instance (states)     out[1]  draws     out[2]  workgroups = wavefronts = draws
 *   out[3]  dynamic LDS bytes     out[4]  launches     out[5]  steps per launch     out[6]  observations
 *   out[7]  spline factors     out[8]  Bernoulli factors
 */
int fokl_assimilate_report(const fokl_ctx *ctx, int64_t *out);

/*
 * out[e * count + j], e < n_draws, j < count: the number the filter draws for draw id draw_ids[e] at point `step` of the
 * time axis for `purpose` and index j.  Philox 4x32-10, key (seed, draw id), counter (step, purpose, index, 2).  Purposes
 * 0 .. 7: the process-noise normal of state `purpose`, index = particle; 8: the normal that spreads the start (step 0,
 * index 64 j + particle); 9: the uniform of the systematic resampling (index 0); 10: the uniform behind the result's
 * draw_index (draw id 0, step 0, index 0).  Host code, no device.  FOKL_ERR_ARG for another purpose.
 */
int fokl_assimilate_rng(uint32_t seed, const uint32_t *draw_ids, int n_draws, uint32_t step, int purpose, int count,
                        double *out);

/* ------------------------------------------------------------------------------------------------------ */
/* Calibration of such a system against measurements (csrc/fokl_calibrate_device.inc; dynamics.py)           */
/* ------------------------------------------------------------------------------------------------------ */

#define FOKL_CALIBRATE_REPORT_LEN 8
#define FOKL_CALIBRATE_WALKERS 128
#define FOKL_CALIBRATE_MAX_UNKNOWN 16

/*
 * What fokl_calibrate_ensemble samples over a fokl_system: d unknowns (initial values of states and constant parameters
 * that enter the models as forcing columns), the measurements and the sampler's settings.  Host memory, row-major.
 */
typedef struct fokl_calibrate_problem {
    int n_unknown;               /* d, 1 .. FOKL_CALIBRATE_MAX_UNKNOWN */
    const int32_t *unknown_src;  /* [d]: >= 0 the state whose initial value unknown i is, -(c + 1) the parameter in forcing
                                  * column c (that column of `forcing` is a placeholder and is never read) */
    const int32_t *norm_param;   /* [n_norm_forcing]: the unknown a forcing input reads, -1: a column of `forcing` */
    const double *lo, *hi;       /* [d] the open box, true scale */
    const double *prior_mean, *prior_prec; /* [d] true scale; precision 0: no prior beyond the box */
    const double *starts;        /* [128, d] strictly inside the box */
    int n_observed;
    const int32_t *obs_state;    /* [n_observed] the state every measured column reads (distinct) */
    const double *obs_hp;        /* [n_observed] 0.5 / obs_sd^2 > 0 */
    int n_obs;
    const int32_t *obs_row;      /* [n_steps + 1]: the row of `data` measured at a point, -1 none; rows appear as 0, 1, ... */
    const double *data;          /* [n_obs, n_observed] true scale, NaN = missing */
    const uint32_t *draw_ids;    /* [n_draws]: the second key word of a draw's random numbers */
    int burnin, draws_kept, thin, jump_every;
    uint32_t seed;
} fokl_calibrate_problem;

/*
 * One affine-invariant ensemble of 128 walkers over the unknowns per posterior draw: which initial states and constant
 * parameters produced the measured run.  A walker's log posterior is -(sum over the present measurements of
 * obs_hp (data - y)^2) - 0.5 sum_i prec_i (theta_i - mean_i)^2 along fokl_simulate_ensemble's trajectory with the draw's
 * coefficients (`system` as fokl_assimilate_ensemble takes it: coef [n_draws, n_coef]); the arithmetic and the sampler are
 * stated by dynamics.calibrate_host (the module docstring of fokl_gpy_amd/dynamics.py): lp is the host's bit for bit.
 *   x_out [n_draws, kept, 128, d], lp_out [n_draws, kept, 128], saturated_out [n_draws, kept, 128] int32 (1: a clamp or the
 *          slope rule acted along the sample's trajectory), kept = ceil(draws_kept / thin); all three or none NULL
 *   sums_out [n_draws, 128, 2, 2, d]: per walker and half of the post-burn-in iterations the sum and the sum of squares of
 *          theta_i - (lo_i + hi_i) / 2; accept_out [n_draws, 128, 2] int32 accepted stretch and jump moves;
 *          evals_out [n_draws] int64 trajectories integrated; invalid_out [n_draws] int32: 1 where a start had no finite lp
 *   trajectories [n_draws, 128, n_states, n_steps + 1] of the final ensemble, or NULL
 * One wavefront per workgroup and draw; lane l is walker l while half 0 moves and walker 64 + l while half 1 moves, so every
 * half step integrates 64 trajectories on 64 lanes.  LDS bytes = (1 + n_factors + n_norm - n_norm_forcing + 7 d) x 64 x 8 +
 * n_coef x 8, at most 144 KB.  No scratch, no atomics: the same arguments give the same bits, and a draw alone equals that
 * draw of a larger call.  The iterations are cut into launches of max(1, FOKL_CALIBRATE_STEPS_PER_LAUNCH / (2 n_steps))
 * iterations (environment, default 65 536 steps): the cut changes no bit.
 * Refused (FOKL_ERR_ARG with a text that names the limit, nothing is launched): what fokl_assimilate_ensemble refuses of a
 * system and of observations, d outside 1 .. 16, an unknown outside the states / the forcing columns, one that no model
 * reads, one named twice, a norm_param that disagrees with unknown_src, an empty or non-finite box, a start that is not
 * strictly inside it, a prior precision that is negative or not finite, thin < 1, draws_kept < 1, burnin < 0 or
 * jump_every < 0 (or above 2^30), the LDS bytes above the budget, outputs beyond the device's free memory
 * (FOKL_CALIBRATE_FREE_BYTES caps what counts as free).  Kernel time: FOKL_K_INTEGRATE.  Blocking.
 */
int fokl_calibrate_ensemble(fokl_ctx *ctx, const fokl_system *system, const fokl_calibrate_problem *problem, double *x_out,
                            double *lp_out, int32_t *saturated_out, double *sums_out, int32_t *accept_out, int64_t *evals_out,
                            int32_t *invalid_out, double *trajectories);

/*
 * The last fokl_calibrate_ensemble call on `ctx`, out [FOKL_CALIBRATE_REPORT_LEN] (host values, no launch); zeros after a
 * call that was refused or failed:
 *   out[0]  NS: the kernel instance (states)     out[1]  draws = workgroups = wavefronts     out[2]  dynamic LDS bytes
 *   out[3]  launches (the replay of the final ensemble included)     out[4]  iterations per launch
 *   out[5]  trajectories integrated, all draws     out[6]  kernel microseconds     out[7]  iterations
 */
int fokl_calibrate_report(const fokl_ctx *ctx, int64_t *out);

/*
 * out[e * count + j], e < n_draws, j < count: the number the sampler draws for draw id draw_ids[e] at `iteration` for
 * `purpose` and index j.  Philox 4x32-10, key (seed, draw id), counter (iteration, purpose, index, 3).  Purposes 0, 1, 2:
 * the uniforms u1, u2, u3 of walker `index` (0 .. 127); 3: the jump move's normal of coordinate i of walker w, index
 * 128 i + w.  Host code, no device.  FOKL_ERR_ARG for another purpose.
 */
int fokl_calibrate_rng(uint32_t seed, const uint32_t *draw_ids, int n_draws, uint32_t iteration, int purpose, int count,
                       double *out);

/* ------------------------------------------------------------------------------------------------------ */
/* Optimal control of such a system, per posterior draw (csrc/fokl_control_device.inc; dynamics.py)          */
/* ------------------------------------------------------------------------------------------------------ */

#define FOKL_CONTROL_REPORT_LEN 8
#define FOKL_CONTROL_MAX_DECISIONS 32
#define FOKL_CONTROL_MAX_STEPS 4096

/*
 * The control problem of fokl_control_solve, fokl_control_pooled_solve and fokl_control_cvar_solve over a fokl_system.
 * Host memory, row-major; D = n_controls x n_segments decision values, d = control x n_segments + segment.
 */
typedef struct fokl_control_problem {
    int n_controls, n_segments;
    const int32_t *seg_first;    /* [n_segments]: the first step of every hold (0 first, increasing, below n_steps) */
    const int32_t *norm_control; /* [n_norm_forcing]: the control a forcing input reads, -1: a column of `forcing` */
    const double *ctl_lo, *ctl_width; /* [n_controls]: u = lo + z width, z in [0, 1] */
    const double *ref;           /* [n_states, n_steps + 1] targets, NaN: not tracked */
    const double *track_weight, *terminal_weight; /* [n_states]: h w_j, and the terminal weights */
    const double *limit_lo, *limit_hi; /* [n_states] (-inf / +inf: open) */
    double limit_weight;         /* h x the soft limits' weight */
    const double *move_weight, *previous; /* [n_controls]; the move of segment 0 counts only with has_previous */
    int has_previous, n_starts;
    const double *z0;            /* [n_starts, D] in [0, 1] */
    int max_iter;                /* 0: the first tangent pass only */
    double tol;                  /* on the projected gradient in z */
} fokl_control_problem;

/*
 * One bounded least-squares solve per (posterior draw, start): projected Gauss-Newton on the cost of dynamics.control, the
 * Jacobian from forward sensitivities of fokl_simulate_ensemble's Runge-Kutta step as executed.  The plan of the system is
 * dynamics._prepare's with the controls as forcing columns (`system` as fokl_assimilate_ensemble takes it: coef
 * [n_draws, n_coef]), the problem is `problem` below, the arithmetic is stated by dynamics.control_host (the module
 * docstring of fokl_gpy_amd/dynamics.py).  Host memory, row-major:
 *   z [n_draws, n_starts, D], cost / cost_start [n_draws, n_starts], status (0 converged, 1 iteration limit, 2 non-finite,
 *          3 stalled) / iterations / descent_steps (iterations whose accepted trial was a steepest-descent lane)
 *          [n_draws, n_starts] int32; best_start [n_draws] int32
 *   members [n_draws, n_states, n_steps + 1]: every draw's trajectory under its best start's controls, first_saturation
 *          [n_draws] int32 of that trajectory
 *   first_F [n_draws, n_starts], first_g [.., D], first_H [.., D, D] (entry [d][d'] as lane d forms it): the tangent pass
 *          of iteration 0; all three or none NULL
 * One wavefront per workgroup and solve, one launch per iteration of every solve (a finished solve returns at once); the
 * statuses are read back every FOKL_CONTROL_POLL launches (environment, default 8; 0: never) to stop queuing early, which
 * changes no result.  LDS bytes = (2 (1 + n_factors + n_norm - n_norm_forcing) + 4 + D) x 64 x 8 + n_coef x 8, at most 144 KB.
 * No atomics: the same arguments give the same bits.
 * Refused (FOKL_ERR_ARG with a text that names the limit, nothing is launched): what fokl_simulate_ensemble refuses of a
 * system (its LDS bound excepted), D above 32, no step or more than 4 096, a control no input reads, an empty or non-finite
 * control box or one outside the training range, negative weights, no residual at all, n_starts < 1, n_draws x n_starts
 * above 1 048 576, a start outside [0, 1], the LDS bytes above.  Kernel time: FOKL_K_INTEGRATE.  Blocking.
 */
int fokl_control_solve(fokl_ctx *ctx, const fokl_system *system, const fokl_control_problem *problem, double *z, double *cost,
                       double *cost_start, int32_t *status, int32_t *iterations, int32_t *descent_steps, int32_t *best_start,
                       double *members, int32_t *first_saturation, double *first_F, double *first_g, double *first_H);

/*
 * The last fokl_control_solve call on `ctx`, out [FOKL_CONTROL_REPORT_LEN] (host values, no launch); zeros after a call
 * that was refused or failed:
 *   out[0]  NS: the kernel instance (states)     out[1]  solves = workgroups = wavefronts     out[2]  D
 *   out[3]  dynamic LDS bytes     out[4]  launches queued     out[5]  launches that found a running solve
 *   out[6]  spline factors     out[7]  Bernoulli factors
 */
int fokl_control_report(const fokl_ctx *ctx, int64_t *out);

/* ------------------------------------------------------------------------------------------------------ */
/* One control sequence for the whole posterior (csrc/fokl_control_pooled_device.inc; dynamics.py)           */
/* ------------------------------------------------------------------------------------------------------ */

#define FOKL_CONTROL_POOLED_REPORT_LEN 15
#define FOKL_CONTROL_POOL_CHUNK 64

/*
 * What iteration 0 of fokl_control_pooled_solve / fokl_control_cvar_solve left in device memory after its last launch, for
 * tests: the trial half of the iteration, which no result shows.  Host memory, row-major, lane = the wavefront's lane (0-30
 * Newton trials, 32-62 steepest-descent trials, 31 and 63 are no trials).  Where the struct is given every pointer that the
 * call uses must be set; a start that stopped before its trial pass (and, in ft, a draw of weight 0) reads NaN, moved 0.
 */
typedef struct fokl_control_first_trial {
    double *trial;    /* [n_starts, D, 64]: the trial points */
    double *slope;    /* [n_starts, 64]: g . (trial - z) */
    int32_t *moved;   /* [n_starts, 64]: the lane is a trial and moves z */
    double *pooled;   /* [n_starts, 2 + D]: F (the CVaR solve: phi), noise and g as the Armijo decision reads them */
    double *ft;       /* [n_starts, n_draws, 64]: every draw's own cost at every trial point */
    double *ft_sums;  /* [n_starts, chunks, 64]: the chunk sums of ft the accept launch adds (pooled solve, alpha == 0) */
    double *phi_t;    /* [n_starts, 64]: phi of every trial point (CVaR solve with alpha > 0) */
    double *a_t;      /* [n_starts, 64]: its a */
    double *z;        /* [n_starts, D]: z after iteration 0 */
    int32_t *status;  /* [n_starts]: after iteration 0; -1 is a start that goes on */
    int32_t *descent; /* [n_starts]: the descent count after iteration 0 */
} fokl_control_first_trial;

/*
 * One bounded least-squares solve per start over ALL draws: the expected cost sum_e w_e F_e(z) of fokl_control_solve's cost,
 * minimised over one decision vector by the same projected Gauss-Newton iteration with the pooled F, noise, g and H in place
 * of one draw's.  The arithmetic is stated by dynamics.control_pooled_host; `system` and `problem` mean what they mean
 * for fokl_control_solve.  Host memory, row-major:
 *   draw_weights [n_draws]: used as given (the caller normalises them to sum 1); a draw of weight 0 is never evaluated
 *   z [n_starts, D], cost / cost_start [n_starts], status / iterations / descent_steps [n_starts] int32; best_start [1] int32
 *   members [n_draws, n_states, n_steps + 1], first_saturation [n_draws] int32: every draw's trajectory under the best
 *          start's controls; cost_draws [n_draws]: every draw's own cost there (one value pass, weight 0 included)
 *   first_pooled [n_starts, n], first_rows [n_starts, n_draws, n] with n = 2 + D + D D: the pooled tangent pass of iteration
 *          0 and the draws' own, each row F, noise, g [D], H [D, D] (entry [d][d'] as lane d forms it); the row of a draw of
 *          weight 0 is NaN; both or none NULL
 *   first_trial: NULL, or what iteration 0 wrote (fokl_control_first_trial above).  NULL changes nothing; otherwise the
 *          buffers it names are filled with NaN before the first launch and the stream is synchronised once after iteration
 *          0's last launch for the copies: the same launches, the same report, the same bits in every other output
 * The pooled sum (dynamics.pooled_sum): chunks of FOKL_CONTROL_POOL_CHUNK consecutive draws, inside a chunk
 * acc = acc + w_e x_e in index order from 0.0, the chunk sums added in chunk order from the first, a draw of weight 0
 * skipped.  One iteration is six launches on the context's stream (tangent pass per (draw, start), chunk sums, Newton step
 * per start, value pass per (draw, start) with lane = trial point, chunk sums, Armijo decision per start); a finished start
 * returns at once in each.  The statuses are read back every FOKL_CONTROL_POLL iterations (environment, default 8; 0:
 * never), which changes no result.  No atomics: the same arguments give the same bits.
 * Refused (FOKL_ERR_ARG with a text that names the limit, nothing is launched): everything fokl_control_solve refuses (the
 * LDS bytes of the per-draw kernels are its formula); a weight that is negative or not finite, weights that sum to zero;
 * a workspace of n_draws x n_starts x (n + 64) x 8 bytes plus (n + 64) x 8 per (start, chunk) beyond the device's free
 * memory, of which FOKL_CONTROL_POOLED_FREE_BYTES (environment) caps what counts.  Kernel time: FOKL_K_INTEGRATE.  Blocking.
 */
int fokl_control_pooled_solve(fokl_ctx *ctx, const fokl_system *system, const fokl_control_problem *problem,
                              const double *draw_weights, double *z, double *cost, double *cost_start, int32_t *status,
                              int32_t *iterations, int32_t *descent_steps, int32_t *best_start, double *members,
                              int32_t *first_saturation, double *cost_draws, double *first_pooled, double *first_rows,
                              const fokl_control_first_trial *first_trial);

/*
 * The last fokl_control_pooled_solve call on `ctx`, out [FOKL_CONTROL_POOLED_REPORT_LEN] (host values, no launch); zeros
 * after a call that was refused or failed:
 *   out[0]  NS: the kernel instance (states)     out[1]  draws     out[2]  starts     out[3]  D     out[4]  chunks
 *   out[5]  dynamic LDS bytes of the per-draw kernels     out[6]  ... of the step kernel
 *   out[7]  iterations queued     out[8]  iterations that found a running start     out[9]  launches per iteration (6)
 *   out[10 .. 14]  with kernel timing enabled, nanoseconds in the tangent, chunk-sum (both), step, trial and accept launches
 */
int fokl_control_pooled_report(const fokl_ctx *ctx, int64_t *out);

/* ------------------------------------------------------------------------------------------------------ */
/* One control sequence that protects the posterior's bad tail (csrc/fokl_control_cvar_device.inc; dynamics.py) */
/* ------------------------------------------------------------------------------------------------------ */

#define FOKL_CONTROL_CVAR_REPORT_LEN 18

/*
 * fokl_control_pooled_solve with the smoothed conditional value at risk at level `alpha` of the draws' costs in place of
 * their weighted mean: phi(z) = min_a a + sum_e w_e s_eps(F_e(z) - a) / (1 - alpha).  The arithmetic is stated by
 * dynamics.control_cvar_host (the risk: dynamics.cvar_smooth); `system`, `problem`, `draw_weights`, and every output up to
 * `cost_draws`, means what it means for fokl_control_pooled_solve, `cost` being phi.  Further, host memory:
 *   alpha in [0, 1); alpha == 0 IS fokl_control_pooled_solve (which is called: first_a reads NaN, first_q the weights,
 *          first_c 0, this call's report stays zero and the pooled call's is written)
 *   epsilon: the width of the smoothed kink in cost units, or NaN for smoothing x the pooled cost of start 0 at its z0 (one
 *          host read after the first tangent launch); fixed for all starts and iterations; epsilon_used [1] returns it
 *   first_pooled [n_starts, n]: phi, noise, g [D], H [D, D] of iteration 0; first_rows as for the pooled solve; first_a
 *          [n_starts]; first_q, first_c [n_starts, n_draws]: the soft tail weights and the band weights; all or none NULL
 *   first_trial: as for fokl_control_pooled_solve, with phi_t and a_t in place of ft_sums; alpha == 0 passes it through
 * One iteration is seven launches: tangent pass per (draw, start), risk per start (min and max, 64 bisections, phi, q, c; one
 * thread per chunk of FOKL_CONTROL_POOL_CHUNK draws), chunk sums under q and c, Newton step per start (adds the band draws'
 * covariance of gradients to H), value pass per (draw, start) with lane = trial point, risk per (start, lane), Armijo
 * decision per start.  Every sum over the draws runs in dynamics.pooled_sum's order.  FOKL_CONTROL_POLL as for the pooled
 * solve; it changes no result.  No atomics: the same arguments give the same bits.
 * Refused (FOKL_ERR_ARG with a text that names the limit): everything fokl_control_pooled_solve refuses; alpha outside
 * [0, 1); a smoothing or an epsilon that is not positive and finite; a relative smoothing where the pooled cost at the start
 * is 0 or not finite (found after the first tangent launch); more draws than the risk kernel's LDS holds ((2 x 64 x chunks +
 * 2 x threads) x 8 bytes within 144 KiB: 141 chunks = 9 024 draws; the kernel's 256 threads are never the limit); a workspace of n_draws x n_starts x (n + 66) x 8 bytes plus
 * (3 + 2 D + 2 D D) x 8 per (start, chunk) plus 64 x (4 + D) x 8 per start beyond the device's free memory, of which
 * FOKL_CONTROL_CVAR_FREE_BYTES (environment) caps what counts.  Kernel time: FOKL_K_INTEGRATE.  Blocking.
 */
int fokl_control_cvar_solve(fokl_ctx *ctx, const fokl_system *system, const fokl_control_problem *problem,
                            const double *draw_weights, double alpha, double smoothing, double epsilon, double *z,
                            double *cost, double *cost_start, int32_t *status, int32_t *iterations, int32_t *descent_steps,
                            int32_t *best_start, double *members, int32_t *first_saturation, double *cost_draws,
                            double *epsilon_used, double *first_pooled, double *first_rows, double *first_a, double *first_q,
                            double *first_c, const fokl_control_first_trial *first_trial);

/*
 * The last fokl_control_cvar_solve call on `ctx` with alpha > 0, out [FOKL_CONTROL_CVAR_REPORT_LEN] (host values, no
 * launch); zeros after a call that was refused, failed or had alpha == 0:
 *   out[0]  NS: the kernel instance (states)     out[1]  draws     out[2]  starts     out[3]  D     out[4]  chunks
 *   out[5]  dynamic LDS bytes of the per-draw kernels     out[6]  ... of the step kernel     out[7]  ... of the risk kernel
 *   out[8]  threads of a risk workgroup     out[9]  iterations queued     out[10]  iterations that found a running start
 *   out[11]  launches per iteration (7)
 *   out[12 .. 17]  with kernel timing enabled, nanoseconds in the tangent, risk (both), chunk-sum, step, trial and accept
 *           launches
 */
int fokl_control_cvar_report(const fokl_ctx *ctx, int64_t *out);

/* ------------------------------------------------------------------------------------------------------ */
/* What the fit kernels ran: K1 basis build, K2 Gram block, K3 residual moments (csrc/fokl_hip.hip)          */
/* ------------------------------------------------------------------------------------------------------ */

/* `which` of fokl_fit_report and the length of each report */
enum { FOKL_REPORT_GRAM = 0, FOKL_REPORT_RESID = 1, FOKL_REPORT_BASIS = 2 };
#define FOKL_GRAM_REPORT_LEN 24
#define FOKL_RESID_REPORT_LEN 10
#define FOKL_BASIS_REPORT_LEN 24
/* out[0] of the Gram report */
enum {
    FOKL_GRAM_NONE = 0,     /* no block yet, or the last call was refused or failed */
    FOKL_GRAM_VALU = 1,     /* gram_valu_kernel + reduce_slabs_kernel (path 1; blocks of at most 64 elements) */
    FOKL_GRAM_TILES = 2,    /* gram_tiles_kernel + reduce_slabs_sym_kernel: the k-split teams of blocks of one or two tiles */
    FOKL_GRAM_DMA = 3,      /* gram_tiles_dma_kernel + reduce_slabs_sym_kernel: every other block */
    FOKL_GRAM_PANEL = 4,    /* gram_mfma_kernel (path 3; development builds) */
    FOKL_GRAM_TILES4 = 5    /* gram_tiles4s_kernel (development builds) */
};
/* out[0] of the residual report; a basis launch's kernel */
enum { FOKL_RESID_NONE = 0, FOKL_RESID_COLUMNS = 1, FOKL_RESID_MATRIX_FREE = 2 };
enum { FOKL_BASIS_NONE = 0, FOKL_BASIS_REG_TABLE = 1, FOKL_BASIS_LDS_TABLE = 2 };

/*
 * What the last launch of a kind on `ctx` ran, out [count] (host; the report's first `count` values):
 * FOKL_REPORT_GRAM, of the last fokl_gram / fokl_gram_launch:
 *   out[0]  the kernel (above)             out[1]  its NT: tiles per wavefront (LDS-DMA: ordinary tiles, NT8)
 *   out[2]  1 = half-tile slots (HALF)     out[3]  loader wavefronts (LW)         out[4]  LDS buffers (0: not LDS-DMA)
 *   out[5]  ks: wavefronts per tile        out[6]  depth: chunks in flight        out[7]  rows per chunk
 *   out[8]  groups (gridDim.y)             out[9]  ct: staged column tiles        out[10] nt: ordinary entries per list
 *   out[11] LDS-DMA pieces per buffer      out[12] dynamic LDS bytes              out[13] the row cut S (gridDim.x)
 *   out[14] chunks the busiest workgroup walks, ceil(chunks / S): above 1 the chunk loop went round
 *   out[15] nr_pad   out[16] nc_pad        out[17] slabs the reduction summed     out[18] its elements per block
 *   out[19] row tiles   out[20] column tiles of the internal order   out[21] lanes per workgroup
 * FOKL_REPORT_RESID, of the last fokl_bic_resid_launch / fokl_bic_resid_terms_launch (and the calls built on them):
 *   out[0]  stored columns or matrix-free  out[1]  columns (matrix-free: terms)   out[2]  batches of RS_BATCH columns: above
 *           1 the table is reloaded per row tile     out[3]  grid     out[4]  row tiles: above the grid the tile loop went round
 *   out[5], out[6]  the matrix-free layout GM x KM   out[7]  its order class (2, 4, 8; 0: splines)   out[8]  its inputs
 * FOKL_REPORT_BASIS, of the last fokl_build_terms / fokl_build_terms_deriv:
 *   out[0]  launches it split into         out[1]  those that ran the LDS-table kernel
 *   out[2 + 7 r ..], r = 0 the first launch, 1 the last, 2 the last LDS-table launch (zeros: there was none):
 *           kernel (above), 1 = splines, lanes per workgroup, distinct factors, spline slabs in LDS, grid, row tiles
 * A call that was refused or failed leaves zeros.  Host values noted while enqueuing: no launch, no synchronisation.
 */
int fokl_fit_report(const fokl_ctx *ctx, int which, int64_t *out, int count);

#ifdef __cplusplus
}
#endif
#endif /* FOKL_HIP_INTERNAL_H */

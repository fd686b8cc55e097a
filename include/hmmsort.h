/*
 * hmmsort.h -- C ABI of libhmmsort_hip.so: the MI355X (gfx950) implementation of the HMM hot
 * path of grero/HMMSpikeSorter.jl (forward/backward/update, viterbi, reconstruct_signal).
 *
 * The reference (Julia) has NO FFI on this path (no ccall anywhere in /root/reference); the
 * boundary is therefore placed at the narrowest existing seam: the Julia methods listed
 * below.  A drop-in keeps their signatures and replaces their bodies by one ccall each
 * (julia/HMMSpikeSorterHIP.jl).  Each entry point cites the reference method
 * it replaces as file:line relative to the reference repository root.
 *
 * Conventions (all inherited from the reference so Julia arrays can be passed as they are):
 *   - matrices are column-major; state ids and transition endpoints are 1-based;
 *   - `states` is the N x S Int16 matrix StateMatrix.states (types.jl:2): entry = row of mu,
 *     1 = silent;
 *   - `tr` is StateMatrix.transitions (types.jl:3): a Vector{Tuple{Int64,Int64,Float64}} is a
 *     contiguous array of 24-byte isbits tuples == struct hmm_trans, in the reference's order
 *     (source-major, destination ascending, types.jl:115-127).  The order is part of the
 *     contract: it fixes Viterbi tie-breaking and log-sum-exp fold order;
 *   - mu is K x N (baumwelch.jl:314); StateMatrix.pi is never read on this path and is not
 *     passed;
 *   - all buffers are owned by the caller; the library reads/writes them only during the call;
 *   - every function returns 0 on success or a negative HMMSORT_E* code and never throws;
 *     hmmsort_last_error() returns a thread-local message for the last failure;
 *   - calls are synchronous (they return after the GPU work and the copy-back finished).
 *     The library is safe to call from several host threads (per-call streams/workspaces).
 *
 * There is no CPU fallback: without a HIP device every compute entry point fails with
 * HMMSORT_EHIP.
 */
#ifndef HMMSORT_H
#define HMMSORT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HMMSORT_OK 0
#define HMMSORT_EINVAL (-1)  /* bad argument / inconsistent model */
#define HMMSORT_ENOMEM (-2)  /* host or device allocation failed / problem too large */
#define HMMSORT_EHIP (-3)    /* HIP runtime error (includes: no device) */
#define HMMSORT_ENOCONV (-4) /* time-parallel engine could not certify its block boundaries */
#define HMMSORT_EUNSUP (-5)  /* model shape not supported by the requested engine */
#define HMMSORT_ENOSILENT (-6) /* chunked decode: a chunk held no silent sample where the stitch rule needs one */

/* Julia Tuple{Int64,Int64,Float64}  (types.jl:3) */
typedef struct hmm_trans {
    int64_t src;
    int64_t dst;
    double lp;
} hmm_trans;

/* engine selection for hmmsort_set_option("engine", ...) */
#define HMMSORT_ENGINE_AUTO 0   /* ring engine when the model is a no-overlap ring model and
                                   T is long enough, else the generic engine */
#define HMMSORT_ENGINE_STRICT 1 /* generic engine: one sequential sweep per signal in the
                                   reference's operation order (bit-exact Viterbi incl. ll) */
#define HMMSORT_ENGINE_RING 2   /* time-parallel ring engine or fail with HMMSORT_EUNSUP */
#define HMMSORT_ENGINE_BLOCKED 3 /* any transition list (overlap models): the strict recursion run
                                    time-parallel over blocks with a certified warm-up */
#define HMMSORT_ENGINE_WAVE 4   /* no-overlap ring models, one wavefront per chain of a few thousand
                                   samples (lane scans; delay lines in LDS); AUTO's choice for ring
                                   models.  HMMSORT_ENGINE_RING = the older lane-per-chain engine */

const char *hmmsort_last_error(void);
int hmmsort_version(void);
int hmmsort_device_count(int *count);
int hmmsort_set_device(int device);
/* keys: "engine" (above), "block" (chain length in samples, 0 = auto), "halo" (warm-up length, 0 = auto),
 *       "escalate" (host-buffer entry points retry with a wider warm-up / the strict engine when a
 *       boundary certificate or the near-tie guard fires; default 1), "plan_cache" (idle plans the
 *       host-buffer entry points keep between calls, default 4, 0 = none), "strict_limit_mb" (largest
 *       back-pointer table the strict fallback of hmmsort_viterbi may allocate, 0 = what is free),
 *       "blocked_hbm_columns" (the blocked E-step and posteriors with their two state columns in device memory
 *       instead of LDS: 0, the default, refuses models past the LDS limit of about 9 900 states as before;
 *       1 sends those models to the device-memory kernels; 2 sends every blocked plan there, for cross-checks.
 *       A plan keeps the value it was created under; values outside 0..2: HMMSORT_EINVAL); read-only
 *       "last_escalations" (retries of the calling thread's last host-buffer call; NEGATIVE = minus the
 *       number of near-tie decisions on a time-parallel path that was returned because the strict sweep's
 *       S x T back-pointers do not fit: the path can differ from the reference's at those decisions only,
 *       whose margins are inside the reference's own rounding noise; hmmsort_last_error has the text;
 *       after a chunked decode: the retries summed over all chunks and channels), "fit_streams" (channels one
 *       worker of hmmsort_fit_channels keeps in flight, each on a stream of its own: default 4, the runtime's
 *       default number of hardware queues; 1..16, HMMSORT_EINVAL outside), "interior" (test aid of the wave
 *       engine, read when a plan is created: 1, the default, lets the forward, Viterbi and backward sweeps run
 *       the full super-steps they own in their interior form; 0 runs every super-step in the general form;
 *       the results are the same bit for bit; 0 or 1, HMMSORT_EINVAL outside).
 * Process-wide defaults behind a mutex; an entry point works on the snapshot it takes when it starts,
 * so options may be changed while other host threads are inside the library.  hmmsort_last_error is
 * per thread. */
int hmmsort_set_option(const char *key, int64_t value);
int hmmsort_get_option(const char *key, int64_t *value);
/* hmmsort_viterbi / hmmsort_em_step leave their plan, workspace and signal buffers in a small cache
 * keyed by (device, T, state matrix, options) and re-arm it on the next call of the same shape (an EM
 * loop, the channels of a recording).  hmmsort_shutdown frees that cache; plans made with
 * hmmsort_plan_create stay the caller's. */
int hmmsort_shutdown(void);

/* ---- state space helpers (host side, no GPU needed) ------------------------------------ */

/* generate_states(N,K,allow_overlaps) .+ 1   (types.jl:65-92,150).  states_out is N x S Int16
 * (1-based rows of mu) or NULL to query S only.  Returns S (>0) or a negative error. */
int64_t hmmsort_generate_states(int64_t N, int64_t K, int allow_overlaps, int16_t *states_out);

/* get_valid_transitions(states, K, lp)  (types.jl:94-127) in closed form: O(R) instead of the
 * reference's O(S^2 N) all-pairs scan, emitting the SAME list in the SAME order with the same
 * floating-point values (log-probabilities are accumulated neuron by neuron exactly as
 * isvalid_transition does).  tr_out may be NULL to query the count.  Returns R or <0.
 * Replaces the rebuild `StateMatrix(states.-1, pp, K, xb[2:end])` of baumwelch.jl:265. */
int64_t hmmsort_build_transitions(int64_t N, int64_t K, const double *lp, int64_t nlp,
                                  int allow_overlaps, hmm_trans *tr_out, int64_t cap);

/* ---- host-buffer entry points: one per reference method ------------------------------- */

/* viterbi(y, lA::StateMatrix, mu, sigma) -> (x::Vector{Int16}, ll)      viterbi.jl:44-98 */
int hmmsort_viterbi(const double *y, int64_t T, const int16_t *states, int64_t N, int64_t K,
                    int64_t S, const hmm_trans *tr, int64_t R, const double *mu, double sigma,
                    int16_t *x_out, double *ll_out);

/* The same decode from the acquisition's raw samples: the reference's CLI converts the int16 channel to
 * Float64 on the host before fit (src/hmmsort.jl:79-88); here the 2-byte samples cross PCIe and are
 * widened in HBM (exact, so the decode is the one hmmsort_viterbi gives on the converted signal). */
int hmmsort_viterbi_i16(const int16_t *y, int64_t T, const int16_t *states, int64_t N, int64_t K,
                        int64_t S, const hmm_trans *tr, int64_t R, const double *mu, double sigma,
                        int16_t *x_out, double *ll_out);

/* ---- chunked decode: fit(HMMSpikingModel, templates, X, chunksize)   fit.jl:11-42, hmmsort.jl:90 ------------
 * The recording is decoded in chunks of `chunksize` samples that depend on each other: the leading non-silent
 * samples of a chunk are skipped (fit.jl:24-28), its trailing ones are left to the next chunk, which starts at
 * the chunk's last silent sample (fit.jl:30-36, :41).  ml_seq starts as all ones; ll is the sum of the chunks'
 * log-likelihoods, added on the host in chunk order; a chunk's value is rounded as the reference rounds it
 * (viterbi.jl:92-96 folded serially along the decoded path on the device), so the sum equals the reference's to
 * the last bit.  The fold is serial (about 3 dependent additions per sample by one thread): measured 3.2 ms per
 * 100 000-sample chunk beside a decode of about 0.8 ms, so one channel runs at 0.20 x the rate of the host loop
 * api.fit, which keeps the engines' own ll (1e-9 relative); channels in step hide part of it.  chunksize <= 0, or one chunk that holds the recording (chunksize >= T > 1): the whole recording
 * in one decode (fit.jl:6-9), exactly hmmsort_viterbi, whose ll keeps 1e-9 relative on the time-parallel engines.
 * T == 1 with chunksize > 0 never enters the loop: ml_seq = [1], ll = 0.
 * The signal is uploaded once (int16 samples as they are, widened in device memory), the stitched path stays in
 * device memory and comes back once; per chunk the host waits once for the chunk's work, reads the chunk's
 * log-likelihood and the two trim points from a pinned record, and then the plan's diagnostics (the engine's own
 * small copies on the idle stream).  Chunk plans (one per chunk length) are made under the options
 * in force and come from / go back to the cache of the host-buffer entry points.  A chunk whose plan reports a
 * failed boundary certificate or open near-ties is decoded again by hmmsort_viterbi's escalation ladder (option
 * "escalate"), as is every chunk of a model with duplicate templates on HMMSORT_ENGINE_RING (no near-tie
 * detector); "last_escalations" is the sum of those retries.
 * Where the reference dies the call returns HMMSORT_ENOSILENT, hmmsort_last_error names the place and the 1-based
 * first sample i of the chunk, and ml_seq_out / ll_out hold what the loop had at that moment:
 *   - fit.jl:26, a chunk that is not the first has no silent sample (BoundsError in the reference): found before
 *     the chunk is written or its log-likelihood added;
 *   - fit.jl:41, a chunk's last silent sample is its first one (or it has none), so the next chunk would not
 *     advance (the reference loops forever): found after the chunk is written and its log-likelihood added.
 * A training step on top of this loop is hmmsort_fit_step_channels (Viterbi training of one or many channels, C = 1
 * included).  Out of scope here: a channels form of the soft hmmsort_em_step, any collective between devices, spike
 * extraction from the resident path, speculative decoding of dependent chunks. */
int hmmsort_fit_chunked(const double *y, int64_t T, int64_t chunksize, const int16_t *states, int64_t N,
                        int64_t K, int64_t S, const hmm_trans *tr, int64_t R, const double *mu, double sigma,
                        int16_t *ml_seq_out, double *ll_out);
int hmmsort_fit_chunked_i16(const int16_t *y, int64_t T, int64_t chunksize, const int16_t *states, int64_t N,
                            int64_t K, int64_t S, const hmm_trans *tr, int64_t R, const double *mu,
                            double sigma, int16_t *ml_seq_out, double *ll_out);

/* the model arguments of hmmsort_viterbi, one record per channel */
typedef struct hmmsort_model {
    const int16_t *states;
    int64_t N, K, S;
    const hmm_trans *tr;
    int64_t R;
    const double *mu;
    double sigma;
} hmmsort_model;

/* The chunked decode of C recording channels of T samples, each with its own model (the reference sorts one
 * channel per call with that channel's templates, hmmsort.jl:79-83; N, K and S may differ between channels).
 * y[c] / ml_seq_out[c]: per-channel host pointers; sample_type HMMSORT_SAMPLES_F64 or HMMSORT_SAMPLES_I16;
 * ll_out: C doubles; status_out: C codes or NULL.  devices == NULL or ndev == 0: everything on the current
 * device, on the calling thread.  Otherwise channel c runs on devices[c % ndev], one worker thread per list
 * position (a device listed twice gets two workers).  The chunks of one channel depend on each other, those of
 * different channels do not: a worker keeps up to option "fit_streams" of its channels in flight, enqueues
 * decode + stitch of each on the channel's own stream, then waits for each, reads and advances.  Options are
 * read once, by the calling thread.  A channel that ends in HMMSORT_ENOSILENT (or another error of its own
 * model) does not stop the others; a HIP or allocation error stops the call.  Returns HMMSORT_OK when every
 * channel is, else the code of the lowest failing channel, whose message goes to the caller's
 * hmmsort_last_error prefixed "channel c:" (0-based).  Each channel's result is what hmmsort_fit_chunked gives
 * for it.  The caller's current device is unchanged. */
int hmmsort_fit_channels(int64_t C, const void *const *y, int sample_type, int64_t T, int64_t chunksize,
                         const hmmsort_model *models, const int *devices, int64_t ndev,
                         int16_t *const *ml_seq_out, double *ll_out, int *status_out);

/* what hmmsort_fit_step_channels returns per channel (pooled: record 0 only) */
typedef struct hmmsort_step_out {
    double *mu;            /* K x N, receives mu' */
    double *sigma;         /* 1 */
    double *lp;            /* lp_cap entries; *n_lp receives the number written (hmmsort_em_step's convention) */
    int64_t lp_cap;
    int64_t *n_lp;         /* may be NULL */
    double *pp;            /* S, may be NULL */
    int64_t *counts;       /* 3 as hmmsort_plan_path_update's d_counts, may be NULL */
} hmmsort_step_out;

/* One step of Viterbi training for C channels over a device list: every channel is decoded exactly as
 * hmmsort_fit_channels decodes it (same arguments, workers, streams, ladder, ml_seq and ll; ml_seq_out or any entry
 * of it may be NULL here), and while its signal and stitched path are still in device memory the path statistics
 * of the whole recording are taken (hmmsort_plan_path_stats on a plan of that channel's model: a chunk plan needs
 * no more than the model) and finished (hmmsort_plan_path_finish).
 *   pooled == 0: each channel is finished with its own model into out[c].
 *   pooled != 0: all models must share N, K, S and the state table (else HMMSORT_EINVAL before any GPU work); the
 *     vectors come to the host, are added in ascending channel order in fp64, go to the device of channel 0 and are
 *     finished there with models[0] into out[0]: one set of templates for all channels.  Any failing channel fails
 *     the call.  x0 adds like every slot, so pp' of a pooled step is no channel's first column: pass pp = NULL.
 * lp_cap too small: HMMSORT_EINVAL.  C = 1 is the hard step inside the chunked native call.  There is no
 * collective inside the library: the vectors are a few hundred KB at most.  No counterpart in the reference. */
int hmmsort_fit_step_channels(int64_t C, const void *const *y, int sample_type, int64_t T, int64_t chunksize,
                              const hmmsort_model *models, const int *devices, int64_t ndev, int pooled,
                              int16_t *const *ml_seq_out, double *ll_out, hmmsort_step_out *out, int *status_out);

/* Drift tracking: how hmmsort_fit_adaptive forgets and when it starts to re-estimate */
typedef struct hmmsort_adapt {
    double halflife;   /* samples after which a statistic weighs 1/2; > 0, +Inf = never forget */
    int64_t warmup;    /* owned samples that must have entered the statistics before the model is first replaced; >= 0 */
    int update_sigma;  /* 0: sigma stays the caller's */
    int update_lp;     /* 0: the transition list stays the caller's, bit for bit */
} hmmsort_adapt;

/* The model track of hmmsort_fit_adaptive: the caller's arrays of `cap` records, one per decoded chunk; any pointer
 * may be NULL.  Chunks beyond cap are counted in *n and not recorded. */
typedef struct hmmsort_track {
    int64_t cap;
    int64_t *n;        /* chunks decoded (all of them, also beyond cap) */
    int64_t *first;    /* [cap]     fit.jl's i of chunk c, 1-based */
    int64_t *own;      /* [cap][2]  0-based range [lo, hi) whose statistics chunk c contributed */
    double *w;         /* [cap]     weight the accumulator was multiplied by before chunk c's statistics were added */
    double *mu;        /* [cap][K*N] the model chunk c was DECODED with */
    double *sigma;     /* [cap] */
} hmmsort_track;

/* The chunked decode with Viterbi training inside the loop: hmmsort_fit_chunked, with the model re-estimated from
 * exponentially weighted path statistics after every chunk, so that templates follow slow changes of the recording
 * (electrode drift).  One channel, host buffers; sample_type HMMSORT_SAMPLES_F64 or HMMSORT_SAMPLES_I16.  No
 * counterpart in the reference.
 * Per chunk the loop is hmmsort_fit_chunked's (plan per chunk length, decode, stitch, the reference-rounded chunk
 * ll, diagnostics, ladder, the HMMSORT_ENOSILENT rules).  After a chunk [i, j] (fit.jl's 1-based i, j) is finished
 * with trim points l, kk (hmmsort_chunk_stitch):
 *   owned range  lo = i + l - 2;  hi = i + kk - 2 when the chunk does not end the recording, hi = T when it does
 *                (0-based, [lo, hi)).  The chunk's last written sample is silent and is the next chunk's first: it is
 *                left out here and the pair (hi-1, hi) reads it.  Samples a later chunk skips (fit.jl:24-28: leading
 *                non-silent samples of a chunk) belong to nobody.
 *   statistics   hmmsort_plan_path_stats over [lo, hi) of the resident signal and stitched path (first = (i == 1)),
 *                blended into the channel's accumulator, which starts at zero, by hmmsort_stats_blend with
 *                w = exp2(-(hi - lo) / halflife) (computed on the host, reported in the track) and plain_tail = 3.
 *   replacement  once the undecayed number of owned samples has reached `warmup`: hmmsort_plan_path_finish of the
 *                accumulator under the current model (rows no sample visited keep their mean); mu <- mu';
 *                sigma <- sigma' if update_sigma (and sigma' is finite and > 0: an accumulator that holds no sample yet
 *                leaves sigma alone); if update_lp the list is rebuilt by hmmsort_build_transitions(N, K, lp', n_lp,
 *                S > 1 + N (K-1)) as after a hard step: non-finite entries leave the list (types.jl:121), so a template
 *                that did not fire within memory can vanish, and on a plan of the generic engines a later lp' is then
 *                shorter than N and the call ends with HMMSORT_EINVAL.  With update_lp == 0 the list is never touched.
 *                The next chunk is decoded with the new model, its ll is taken under it.
 * ll_out: the sum of the chunks' reference-rounded values, each under the model that chunk was decoded with.
 * track (may be NULL): record c describes chunk c; with a stationary signal the path is hmmsort_fit_chunked's only
 * as far as the re-estimated templates decode it alike.  final_model (may be NULL; mu, sigma, lp required as in
 * hmmsort_fit_step_channels): the full finish of the accumulator after the last chunk under the last model -- mu',
 * sigma', lp', pp', counts, whatever warmup, update_sigma and update_lp say.
 * chunksize <= 0, or one chunk that holds the recording: exactly hmmsort_fit_chunked's result, *track->n = 1 with
 * own = [0, T), final_model from the statistics of [0, T).  T == 1: [1], ll = 0, *track->n = 0.
 * HMMSORT_ENOSILENT: ml_seq_out, ll_out and the track hold what the loop had (records of the chunks that were
 * finished); final_model is not written.  halflife <= 0 or NaN, warmup < 0, opt == NULL: HMMSORT_EINVAL before any
 * GPU work.  The range comes from l and kk, so the loop waits for the device twice per chunk. */
int hmmsort_fit_adaptive(const void *y, int sample_type, int64_t T, int64_t chunksize, const hmmsort_model *model,
                         const hmmsort_adapt *opt, int16_t *ml_seq_out, double *ll_out, hmmsort_track *track,
                         hmmsort_step_out *final_model /* may be NULL: the model after the last chunk */);

/* forward(V, lA::StateMatrix, mu, sigma) -> alpha (S x T)            baumwelch.jl:25-51 */
int hmmsort_forward(const double *y, int64_t T, const int16_t *states, int64_t N, int64_t K,
                    int64_t S, const hmm_trans *tr, int64_t R, const double *mu, double sigma,
                    double *alpha_out);

/* backward(V, lA::StateMatrix, mu, sigma) -> beta (S x T)            baumwelch.jl:73-98 */
int hmmsort_backward(const double *y, int64_t T, const int16_t *states, int64_t N, int64_t K,
                     int64_t S, const hmm_trans *tr, int64_t R, const double *mu, double sigma,
                     double *beta_out);

/* update(alpha, beta, lA, mu, sigma, x) -> (StateMatrix, mu, sigma)  baumwelch.jl:205-309
 * mu_inout (K x N) is zeroed and rewritten in place as the reference does (:268).
 * lp_out receives xb[2:end] (:264-265): n_lp_out = (#transitions with src == 1) - 1 values
 * (== N without overlaps); pp_out receives gammaf[:,1] (S values).  The new StateMatrix is
 * rebuilt by the caller from lp_out (hmmsort_build_transitions or the reference constructor). */
int hmmsort_update(const double *alpha, const double *beta, const double *x, int64_t T,
                   const int16_t *states, int64_t N, int64_t K, int64_t S, const hmm_trans *tr,
                   int64_t R, double *mu_inout, double sigma, double *sigma_out, double *lp_out,
                   int64_t lp_cap, int64_t *n_lp_out, double *pp_out);

/* train_model(X, state_matrix, mu0, sigma0) = forward -> backward -> update
 *                                                                    baumwelch.jl:362-370
 * Same outputs as hmmsort_update; alpha/beta are never materialised by the ring engine. */
int hmmsort_em_step(const double *y, int64_t T, const int16_t *states, int64_t N, int64_t K,
                    int64_t S, const hmm_trans *tr, int64_t R, double *mu_inout, double sigma,
                    double *sigma_out, double *lp_out, int64_t lp_cap, int64_t *n_lp_out,
                    double *pp_out);

/* One step of Viterbi training: hmmsort_viterbi, then hmmsort_plan_path_update on the signal and path that are
 * already in device memory.  Argument conventions of hmmsort_em_step (mu_inout rewritten in place, n_lp_out,
 * lp_cap too small: HMMSORT_EINVAL); same plan cache and escalation ladder as hmmsort_viterbi, the update runs on
 * whatever path the ladder finally returned, and "last_escalations" means what it means there.  x_out (T) and
 * ll_out receive the decode of the OLD model; either may be NULL.  No counterpart in the reference. */
int hmmsort_viterbi_step(const double *y, int64_t T, const int16_t *states, int64_t N, int64_t K, int64_t S,
                         const hmm_trans *tr, int64_t R, double *mu_inout, double sigma, double *sigma_out,
                         double *lp_out, int64_t lp_cap, int64_t *n_lp_out, double *pp_out,
                         int16_t *x_out /* may be NULL */, double *ll_out /* may be NULL */);

/* reconstruct_signal(x, lA, mu, sigma) -> Y2 (sigma is ignored)    reconstruction.jl:1-10 */
int hmmsort_reconstruct(const int16_t *x, int64_t T, const int16_t *states, int64_t N,
                        int64_t S, const double *mu, int64_t K, double *y_out);

/* reconstruct_signal under a model track (hmmsort_fit_adaptive's): y2[t] = sum_l mu_c(t)[states[l, x_t], l], where
 * c(t) is the last chunk whose first sample is <= t.  first: nchunks 1-based sample numbers, strictly ascending
 * (at most 8192; HMMSORT_EUNSUP beyond); mu_track: [nchunks][K*N].  State ids outside 1..S, and samples before
 * first[0], give NaN (the device code's answer; hmmsort_reconstruct refuses such ids on the host).  No counterpart
 * in the reference. */
int hmmsort_reconstruct_tracked(const int16_t *x, int64_t T, const int16_t *states, int64_t N, int64_t S, int64_t K,
                                int64_t nchunks, const int64_t *first /* 1-based, ascending */,
                                const double *mu_track /* [nchunks][K*N] */, double *y_out);

/* unroll_mlseq(mlseq, state_matrix) -> N x T Int16                   extraction.jl:4-13 */
int hmmsort_unroll_mlseq(const int16_t *mlseq, int64_t T, const int16_t *states, int64_t N,
                         int64_t S, int16_t *out);

/* extract_spiketimes(model)                                              extraction.jl:15-24
 * For neuron i the spike time is every sample whose decoded state has neuron i at the row of its
 * template minimum (indmin(mu[:,i]), first minimum).  times_out is N rows of `cap` entries
 * (1-based sample indices, ascending, as Julia's findin returns them); counts_out[i] is the total
 * number found (entries beyond cap are dropped: call again with a larger cap). */
int hmmsort_extract_spiketimes(const int16_t *mlseq, int64_t T, const int16_t *states, int64_t N,
                               int64_t S, const double *mu, int64_t K, int64_t *times_out,
                               int64_t cap, int64_t *counts_out);

/* ---- device-resident plan API --------------------------------------------------------- */
/* Used by bench.py and by multi-GPU hosts: the signal stays in HBM, the caller owns device
 * buffers (plain device pointers) and the HIP stream (passed as void* == hipStream_t; NULL =
 * the null stream).  No call below synchronises the stream unless noted. */

typedef struct hmmsort_plan hmmsort_plan;

/* Analyse the model, pick the engine and allocate the device workspace for signals of length T
 * (one recording channel).  Synchronous. */
int hmmsort_plan_create(hmmsort_plan **plan_out, int64_t T, const int16_t *states, int64_t N,
                        int64_t K, int64_t S, const hmm_trans *tr, int64_t R, const double *mu,
                        double sigma);
/* Batched plan (SURVEY 8b "batched variants with a leading channel count C"): C recording channels of
 * the same length T and the same model shape, each with its own transition values, templates and sigma
 * (the reference sorts one channel per call with that channel's model, src/hmmsort.jl:79-83).
 *   tr: C lists of R records, mu: C matrices of K x N, sigma: C values.
 * Every plan call then takes channel-major device buffers: d_y [C][T], d_x [C][T], d_ll [C],
 * d_stats [C][hmmsort_plan_stats_len()], d_out [C][K*N + 1 + N + S]; one set of launches sweeps all
 * channels (chains = channels x chains per channel), so short channels still fill the GPU.  Summing the
 * per-channel statistics before hmmsort_plan_mstep gives pooled templates (an extension the reference
 * lacks).  Wave engine only (HMMSORT_EUNSUP otherwise); diagnostics are summed over the channels. */
int hmmsort_plan_create_batched(hmmsort_plan **plan_out, int64_t C, int64_t T, const int16_t *states,
                                int64_t N, int64_t K, int64_t S, const hmm_trans *tr, int64_t R,
                                const double *mu, const double *sigma);
int64_t hmmsort_plan_channels(const hmmsort_plan *plan);
/* hmmsort_plan_set_model for one channel of a batched plan */
int hmmsort_plan_set_model_channel(hmmsort_plan *plan, int64_t channel, const hmm_trans *tr, int64_t R,
                                   const double *mu, double sigma);
/* Replace transitions / mu / sigma (same N, K, S; R may shrink when a template has lost its entry
 * transitions) -- e.g. between EM iterations. */
int hmmsort_plan_set_model(hmmsort_plan *plan, const hmm_trans *tr, int64_t R, const double *mu,
                           double sigma);
int hmmsort_plan_destroy(hmmsort_plan *plan);
/* engine actually used (HMMSORT_ENGINE_STRICT or HMMSORT_ENGINE_RING), geometry, bytes */
int hmmsort_plan_info(const hmmsort_plan *plan, int64_t *engine, int64_t *block, int64_t *halo,
                      int64_t *nchains, int64_t *workspace_bytes);
/* Overlap models on the blocked engine: which sweep the plan's current model runs -- 0 the generic sweeps (any
 * transition list), 2 the two-template sweep (csrc/pair_sweep.hip), 3..5 the multi-template sweep (csrc/multi_sweep.hip);
 * it follows hmmsort_plan_set_model and drops to 0 when a host entry point fell back.  Other engines: 0. */
int64_t hmmsort_plan_overlap_sweep(const hmmsort_plan *plan);

/* Optional: compute the signal-dependent intermediates every ring-engine call needs (transposed
 * copy of y and the ring scores of the current model) ONCE and let the following
 * hmmsort_plan_viterbi / hmmsort_plan_estep calls on the same d_y reuse them.  The binding ends at
 * hmmsort_plan_set_model, hmmsort_plan_unbind or a call with a different pointer.  The caller
 * promises not to modify d_y while it is bound.  No-op for the generic engine. */
int hmmsort_plan_bind(hmmsort_plan *plan, const double *d_y, void *stream);
int hmmsort_plan_unbind(hmmsort_plan *plan);

/* Viterbi decode of d_y[0..T) into d_x[0..T) (device Int16).  d_ll: one device double. */
int hmmsort_plan_viterbi(hmmsort_plan *plan, const double *d_y, int16_t *d_x, double *d_ll,
                         void *stream);
/* E-step: forward-backward + sufficient statistics.  d_stats receives
 * hmmsort_plan_stats_len() doubles (layout: hmmsort_plan_stats_layout below); the vector is a
 * plain sum over time, so shards of one recording / pooled channels combine by a SUM
 * all-reduce (RCCL) before the M-step. */
int hmmsort_plan_estep(hmmsort_plan *plan, const double *d_y, double *d_stats, void *stream);
/* hmmsort_plan_viterbi + hmmsort_plan_estep of the same signal and model in one call: the three
 * serial sweeps (Viterbi, forward, backward) are independent and share one launch, so three times
 * as many wavefronts are resident (wave engine: the Viterbi sweep and its post-processing run on an
 * internal stream beside the forward/backward sweeps).  Same results as the two separate calls.
 * Wave and ring engines. */
int hmmsort_plan_decode_estep(hmmsort_plan *plan, const double *d_y, int16_t *d_x, double *d_ll,
                              double *d_stats, void *stream);
int64_t hmmsort_plan_stats_len(const hmmsort_plan *plan);
/* Time-sharding ONE recording over several plans/GPUs: the plan's signal is the slice
 * [own_lo - halo_before, own_hi + halo_after) of the recording (halos of >= a few ring lengths;
 * the slice's own ends act as warm-up), and the E-step accumulates statistics only for samples /
 * ring onsets in [own_lo, own_hi) (slice coordinates).  `first` / `last` say whether the slice
 * starts / ends the recording (the reference's first-column and terminal conditions apply there).
 * Summing the statistics of all shards (SUM all-reduce) and calling hmmsort_plan_mstep gives the
 * EM step of the whole recording.  pp (gamma[:,1]) is meaningful on the first shard only.
 * Default: the plan owns everything (one shard = the recording). */
int hmmsort_plan_set_shard(hmmsort_plan *plan, int64_t own_lo, int64_t own_hi, int first, int last);
/* M-step finish from (all-reduced) statistics, on device: d_out receives
 * [mu (K*N) | sigma (1) | lp_new | pp (S)]; lp_new = xb[2:end] (baumwelch.jl:264) has one entry per
 * transition leaving state 1 except the first: N entries for models without overlaps.  Blocked plans
 * (overlap models) take the same three calls estep / all-reduce / mstep; their statistics vector is
 * [G0 (S) | G1 (S) | X | Gamma0 | sum y^2]. */
int hmmsort_plan_mstep(hmmsort_plan *plan, const double *d_stats, double *d_out, void *stream);
/* Viterbi training (hard EM; INTEGRATION.md "Viterbi training"): the model re-estimated from a path
 * d_x of d_y, normally the one hmmsort_plan_viterbi just wrote.  It is update() (baumwelch.jl:205-309) with gamma
 * and xi the indicators of the path: mu'[k,l] = mean of y over the samples whose state has template l alone active,
 * at phase k (samples in states with two or more active templates do not enter mu, baumwelch.jl:269-287; a row
 * (k,l) no sample visits keeps the plan's current value instead of 0/0); sigma' = sqrt(mean (y - _mu'[x])^2) with
 * the NEW means, over all states; lp'_i = log(#(1 -> dst_i)) - log(#(x_t = 1, t < T-1)) for the transitions out of
 * state 1 but the first, -Inf for a count of 0; pp' = 0 at x_0, -Inf elsewhere.  d_out per channel is
 * hmmsort_plan_mstep_len() doubles in hmmsort_plan_mstep's layout.  d_counts (may be NULL) receives three device
 * int64 per channel: [0] samples with an id outside 1..S (skipped everywhere), [1] pairs (x_t, x_t+1) that are no
 * transition of the list -- the path is then not one of this model and d_out is unspecified, though the call stays
 * inside its buffers and finishes --, [2] rows (k,l) that kept their mean.  Any plan (wave, ring, blocked, strict,
 * batched: channel-major buffers); a time shard (hmmsort_plan_set_shard with anything but the whole recording):
 * HMMSORT_EINVAL, because sigma' needs the means of the whole recording.  No floating-point atomics: the same
 * inputs give the same bits.  Asynchronous on `stream`. */
int hmmsort_plan_path_update(hmmsort_plan *plan, const double *d_y, const int16_t *d_x, double *d_out,
                             int64_t *d_counts, void *stream);
/* The same update from additive statistics, for time shards, chunked paths and pooled channels.
 * hmmsort_plan_path_stats takes the statistics of samples [own_lo, own_hi) of the arrays d_y / d_x of length T.
 * T is the length of the ARRAYS, not of the plan: the call uses the plan's model and nothing of its engine, so a
 * plan of chunk length serves the stitched path of a whole recording (workspace grows on demand).  Batched plans
 * take channel-major [C][T] arrays and T must be the plan's (HMMSORT_EINVAL otherwise).  The range is explicit and
 * independent of hmmsort_plan_set_shard, so it exists on blocked and strict plans too; 0 <= own_lo <= own_hi <= T
 * (else HMMSORT_EINVAL), an empty range gives a zero vector.  Pairs (t, t+1) are counted for t owned and t+1 < T:
 * an interior shard reads x[own_hi] in its halo and owns that pair.  `first`: the arrays start the recording.
 * d_stats receives hmmsort_plan_path_stats_len() doubles PER CHANNEL, with NE = N (K-1) and n_lp as in
 * hmmsort_plan_mstep_len:
 *   [ c (NE) | s (NE) | sm (NE) | n_j (S) | ent (n_lp) | b | sum_y2 | n | x0 | bad0 | bad1 ]    3 NE + S + n_lp + 6
 *   c, s    count and sum of y per entry e = l (K-1) + (k-2) over samples whose state has template l alone, at phase k
 *   sm      sum of y over samples in states with two or more active templates, entered once per active template
 *   n_j     samples in each such state j (0 for the other states)
 *   ent, b  the counts behind lp': transitions 1 -> dst_i, and samples in state 1 that have a successor
 *   sum_y2, n   over the owned samples with a valid id;  bad0, bad1: counts [0] and [1] of hmmsort_plan_path_update
 *   x0      the id x[0] when `first`, own_lo == 0 and the id is valid, else 0
 * Counts are doubles (exact to 2^53), so the vectors of shards, chunks or channels add in any order without error
 * in the integer slots: SUM all-reduce, or hmmsort_stats_sum.  No floating-point atomics: the vector is a fixed
 * function of (y, x, model, range).
 * hmmsort_plan_path_finish turns one such vector per channel and the plan's current model (kept rows, slot order)
 * into d_out / d_counts as hmmsort_plan_path_update writes them.  sigma'^2 = (sum_y2 - 2 sum_e mu'_e (s_e + sm_e)
 * + sum_e c_e mu'_e^2 + sum_j n_j M_j^2) / n with M_j the state means of the new templates, clamped at 0.
 * For own = [0, T), first = 1 and T the plan's, mu', lp', pp' and the counts equal hmmsort_plan_path_update's bit
 * for bit (same tiles, same order); sigma' agrees within the rounding of the four sums.
 * One statistics call at a time per plan (they share its workspace).  All asynchronous on `stream`, except that the
 * first call after plan creation or hmmsort_plan_set_model waits for `stream` once, behind the upload of its tables. */
int64_t hmmsort_plan_path_stats_len(const hmmsort_plan *plan);              /* per channel */
int hmmsort_plan_path_stats(hmmsort_plan *plan, const double *d_y, const int16_t *d_x, int64_t T, int64_t own_lo,
                            int64_t own_hi, int first, double *d_stats, void *stream);
int hmmsort_plan_path_finish(hmmsort_plan *plan, const double *d_stats, double *d_out, int64_t *d_counts,
                             void *stream);
/* d_out[i] = d_parts[0][i] + d_parts[1][i] + ... in ascending order, for nparts contiguous device vectors of len
 * doubles: the on-device, fixed-order alternative to an all-reduce, for any statistics vector of the library. */
int hmmsort_stats_sum(const double *d_parts, int64_t nparts, int64_t len, double *d_out, void *stream);
/* Exponentially weighted statistics, in place on device vectors of len doubles: d_acc[i] = w * d_acc[i] + d_new[i]
 * for i < len - plain_tail, the product rounded, then the sum rounded (never a fused multiply-add: two IEEE
 * operations on the host give the same bits); d_acc[i] += d_new[i] for the last plain_tail entries.  A
 * path-statistics vector takes plain_tail = 3: x0, bad0 and bad1 are an identifier and diagnostics, not weights.
 * One thread per entry, asynchronous on `stream`.  w outside [0, 1] or NaN, len < plain_tail, plain_tail < 0:
 * HMMSORT_EINVAL. */
int hmmsort_stats_blend(double *d_acc, double w, const double *d_new, int64_t len, int64_t plain_tail, void *stream);
/* doubles hmmsort_plan_mstep writes PER CHANNEL: K*N + 1 + n_lp + S, n_lp = N for wave/ring plans (also when
 * the list has lost a vanished template's entry transitions, types.jl:121: its slot stays, value -Inf or the
 * re-estimate), (#transitions leaving state 1) - 1 for the blocked engine (baumwelch.jl:226,264). */
int64_t hmmsort_plan_mstep_len(const hmmsort_plan *plan);
/* diagnostics of the last time-parallel call on this plan (synchronises the stream):
 * diag[0] = chain boundaries whose Viterbi warm-up missed the certificate (the warm-up's boundary
 *           scores must equal the previous chain's up to one constant; ring engine 1e-6 on the
 *           relevant entries, wave engine 1e-9 on all 1 + N L entries).  The wave engine re-sweeps a
 *           failing chain exactly from its predecessor's hand-off and counts only boundaries still
 *           open after two such rounds,
 * diag[1] = backtrace stitch repairs (wave engine: + chains re-swept exactly), diag[2] = largest spread seen by that certificate (bit
 *           pattern of a double), diag[3] / diag[5] = chain boundaries whose forward / backward warm-up
 *           missed the posterior-weighted tolerance 1e-9, diag[4] / diag[6] = the largest such
 *           error (IEEE-754 bit pattern of a double).  Viterbi calls fill [0..1], E-step calls
 *           [3..6] (blocked plans: [3..6] from the certificates on gamma of generic_estep.hip).
 *           Blocked engine: diag[0], diag[2] as above for its block boundaries, and
 *           diag[7] = blocks in which two candidates of a maximum came closer than the rounding
 *           granularity of the reference's trellis at that point (near-ties, e.g. duplicate
 *           templates): the blocks' additive frames may then break a tie the reference breaks by
 *           list order; hmmsort_viterbi re-decodes such signals with the strict engine.
 *           Wave engine: junction decisions whose margin is below 16 (L+2) ulp(|T1|max) + 4e-9 (the most the
 *           reference's own rounding can move a difference at the magnitude its trellis reaches on this
 *           signal) are flagged, and the flagged ones ON the decoded path are re-decided on device with the
 *           reference's serial arithmetic (hmmsort_plan_tie_stats); diag[7] = decisions that could NOT be
 *           settled that way (0 on every signal seen; same consequence as above otherwise). */
int hmmsort_plan_diagnostics(hmmsort_plan *plan, void *stream, int64_t diag[8]);

/* Wave engine: what the exact near-tie resolver did in the last decode (synchronises the stream), summed
 * over the channels: out[0] flagged junction decisions the backtrace met (trigger), out[1] flagged decisions
 * on the final path, out[2] decisions re-decided with the reference's serial arithmetic (viterbi.jl:74-84;
 * includes flagged decisions off the path that a candidate's own history ran through), out[3] decisions
 * whose back-pointer changed, out[4] decisions left unresolved (== diag[7]), out[5] channels whose final
 * arg-max (viterbi.jl:90) was flagged, out[6] longest candidate walk in samples (max), out[7] blocks of the
 * exact prefix that were folded serially.  Zeros for other engines. */
int hmmsort_plan_tie_stats(hmmsort_plan *plan, void *stream, int64_t out[8]);

/* reconstruct_signal (reconstruction.jl:1-10) and unroll_mlseq (extraction.jl:4-13) of a decoded
 * path in device memory into device buffers (T doubles / N x T Int16, column-major); the model
 * is the plan's current one.  Out-of-range state ids give NaN / 0 as in the host-buffer kernels'
 * device code; synchronise the stream. */
int hmmsort_plan_reconstruct(hmmsort_plan *plan, const int16_t *d_x, double *d_y_out, void *stream);
int hmmsort_plan_unroll_mlseq(hmmsort_plan *plan, const int16_t *d_x, int16_t *d_out, void *stream);

/* extract_spiketimes (extraction.jl:15-24) on a decoded path that is still in device memory
 * (the x written by hmmsort_plan_viterbi): only the spike times cross PCIe, not the 2 bytes per
 * sample of the path.  Model (states, mu) = the plan's current one.  Host outputs as in
 * hmmsort_extract_spiketimes; synchronises the stream. */
int hmmsort_plan_extract_spiketimes(hmmsort_plan *plan, const int16_t *d_x, int64_t *times_out,
                                    int64_t cap, int64_t *counts_out, void *stream);

/* Smoothed state posteriors gamma_t(s) = P(state s at sample t | whole recording) of the plan's current
 * model(s), left in device memory (definitions: INTEGRATION.md "Posteriors"; an extension, the reference keeps
 * the decoded path only).  Per channel of a batched plan (channel-major like every plan buffer):
 *   d_onset  [C][N][T]  mass of the states in which template a is at its first phase (states[a,s] == 2)
 *   d_occ    [C][N][T]  mass of the states in which template a is mid-spike (states[a,s] > 1)
 *   d_silent [C][T]     mass of state 1
 *   d_logz   [C]        log-likelihood of the recording, logsumexp_s alpha_{T-1}(s)
 * Any output may be NULL.  Wave plans (ring models, up to 16 templates) run the forward sweep, the unfused
 * backward sweep and one streaming pass.  Blocked plans (overlap models; option "engine" =
 * HMMSORT_ENGINE_BLOCKED, or AUTO from 4 096 samples) run the time-parallel E-step's sweep with the per-sample
 * marginals kept: no S x T array, asynchronous on `stream`; the model must fit the blocked E-step (two columns
 * of S doubles within 156 KB of LDS, about 9 900 states) and have at most 4 templates, else HMMSORT_EUNSUP
 * naming the limit.  A plan created under option "blocked_hbm_columns" = 1 or 2 keeps the columns in device
 * memory and takes any number of states (the reference's 3- and 4-template overlap models at K = 60 have
 * 10 621 and 21 123), still at most 4 templates and 256 transitions out of the silent state; its workspace, a
 * window of block x S doubles per resident workgroup, is capped at half of the free device memory and reported
 * by hmmsort_plan_info (HMMSORT_ENOMEM naming the bytes when not even one workgroup fits).  Strict plans (any model; option "engine" = HMMSORT_ENGINE_STRICT) materialise alpha and
 * beta (2 x S x T doubles, bounded by "strict_limit_mb": HMMSORT_ENOMEM beyond it) and synchronise the stream.
 * Ring-engine plans: HMMSORT_EUNSUP.  A time shard (hmmsort_plan_set_shard; wave plans only): HMMSORT_EINVAL.
 * The warm-up certificates of a wave or blocked plan run and count into hmmsort_plan_diagnostics (diag[3..6])
 * as in an E-step; a caller that sees diag[3] or diag[5] != 0 widens option "halo" and repeats the call.
 * The plan keeps the posteriors for the three calls below until its next E-step, hmmsort_plan_set_model or
 * posterior call. */
int hmmsort_plan_posteriors(hmmsort_plan *plan, const double *d_y, double *d_onset, double *d_occ,
                            double *d_silent, double *d_logz, void *stream);
/* Maximum-posterior-marginal decode: d_xm[t] = arg max_s gamma_t(s), 1-based like the Viterbi path, ties to
 * the lower state number.  [C][T] Int16 in device memory. */
int hmmsort_plan_posterior_decode(hmmsort_plan *plan, int16_t *d_xm, void *stream);
/* Confidence of every spike of a decoded path d_x ([C][T], normally hmmsort_plan_viterbi's): for each event
 * hmmsort_plan_extract_spiketimes reports for template a at sample t, the posterior probability that template a
 * was in its trough state within +-jitter samples of t, min(1, sum_{|d| <= jitter} gamma_{t+d}(trough of a)).
 * times_out / conf_out: [C][N][cap] on the host, counts_out [C][N]; protocol of hmmsort_extract_spiketimes
 * (cap = 0 counts only).  Synchronises the stream. */
int hmmsort_plan_spike_confidence(hmmsort_plan *plan, const int16_t *d_x, int64_t jitter, int64_t *times_out,
                                  double *conf_out, int64_t cap, int64_t *counts_out, void *stream);
/* Expected number of spikes per template, sum_t onset[a,t] (events whose first phase falls inside the
 * recording).  counts_out: [C][N] on the host.  Synchronises the stream. */
int hmmsort_plan_expected_counts(hmmsort_plan *plan, double *counts_out, void *stream);
/* Host-buffer form (model arguments as hmmsort_em_step, same plan cache and escalation): onset / occ (N x T,
 * template-major), silent (T), xm (T), logz (1); NULL skips an output.  A model the wave engine does not take
 * runs on the strict engine, unless option "engine" is HMMSORT_ENGINE_BLOCKED and the model fits the blocked
 * posterior path: then on the blocked engine, whose failed certificates widen the warm-up (counted in option
 * "last_escalations") and finally fall back to the strict engine. */
int hmmsort_posteriors(const double *y, int64_t T, const int16_t *states, int64_t N, int64_t K, int64_t S,
                       const hmm_trans *tr, int64_t R, const double *mu, double sigma, double *onset,
                       double *occ, double *silent, int16_t *xm, double *logz);

/* Per-spike amplitude and residual, and a per-template quality summary (an extension): how well the
 * spike the path placed fits the samples under it, once the other templates the path says are active are taken out.
 * Inputs: y[T] (fp64, or int16 widened exactly), x[T] an Int16 path, 1-based (normally a decode; any array is
 * accepted), states N x S, mu K x N, and optionally a model track (nchunks, first, mu_track) as
 * hmmsort_reconstruct_tracked takes it; nchunks == 0: no track.
 *   events    exactly those of hmmsort_extract_spiketimes, in its ascending order: template a has an event at 0-based
 *             sample t when x[t] is in 1..S and states[a, x[t]] == qv_a, the trough value of the BASE mu (also under a
 *             track).  A template whose minimum is in the silent row (qv_a == 1): HMMSORT_EINVAL naming it.
 *   model     M = mu; under a track M = mu_track[c] for the last chunk c with first[c] <= t + 1 (the trough's chunk
 *             serves the whole window).  An event before first[0]: amp = rss = energy = NaN, nused = 0; it is counted
 *             in n only.
 *   window    for phases k = 2..K ascending, u = t + (k - qv_a); phase k is used iff 0 <= u < T, x[u] is in 1..S and
 *             states[a, x[u]] == k (a path that jumps, starts or ends mid-spike gives a partial event).  nused = number
 *             of used phases; the event is full iff nused == K - 1.
 *   phase     oth = 0.0; for b ascending, b != a: oth += M[states[b, x[u]] - 1, b] (reconstruct_signal's row lookup,
 *             silent row included);  r = y[u] - oth;  m = M[k - 1, a].
 *   event     four serial folds from 0.0 in ascending k, product and sum rounded separately (never a fused
 *             multiply-add): srm += r*m, smm += m*m, energy += r*r, rss += d*d with d = r - m.  amp = srm / smm, the
 *             IEEE quotient whatever it is.  rss is the residual at unit amplitude; the residual at the fitted
 *             amplitude is energy - amp * srm = energy - amp * amp * smm and is left to the caller.
 *   summary   per template 8 + 3 (K-1) doubles: [0] n (all events), [1] n_full, [2] sum amp, [3] sum amp*amp,
 *             [4] sum rss, [5] sum energy (2..5 over full events), [6] sum nused (all events), [7] smm of the whole base
 *             template (k = 2..K ascending); then wsum, wsq, wcnt of K-1 entries each: sum of r, sum of r*r and count
 *             per phase over every used phase of every event -- the overlap-cleaned spike-triggered mean and spread, what
 *             one compares a template loaded from a file against.  Fixed order, no floating-point atomics: events in
 *             ascending order are cut into blocks of 256, each slot's block partial is a serial fold from 0.0 in event
 *             order, the partials are folded serially from 0.0 in block order; counts are doubles.  The summary covers
 *             all n events, also when cap < n.
 * Outputs are host arrays: times (1-based), amp, rss, energy, nused as N rows of `cap` entries, any of them NULL;
 * counts [N] is required; protocol of hmmsort_extract_spiketimes (entries beyond cap are dropped, entries beyond counts
 * untouched; cap = 0: counts and summary only).
 * Refused before any GPU work: a null required argument, N outside 1..32, K < 2, a sample type other than F64 / I16,
 * first not strictly ascending or first[0] < 1 (HMMSORT_EINVAL); nchunks > 8192 (HMMSORT_EUNSUP).  T == 0: zero counts,
 * zero summary except [7].
 * hmmsort_spike_fit: host buffers, no plan; uploads once, int16 samples as they are (widened on the device).
 * hmmsort_plan_spike_fit: resident d_y / d_x of the plan's length under the plan's current model; a batched plan takes
 * channel-major buffers and writes [C][N][cap], [C][N] and [C][N][8 + 3 (K-1)] as hmmsort_plan_spike_confidence lays
 * them out, and takes no track (HMMSORT_EINVAL).  Synchronises the stream. */
typedef struct hmmsort_spike_fit_out {
    int64_t *times;     /* [N][cap], may be NULL */
    double *amp;        /* [N][cap], may be NULL */
    double *rss;        /* [N][cap], may be NULL */
    double *energy;     /* [N][cap], may be NULL */
    int32_t *nused;     /* [N][cap], may be NULL */
    int64_t cap;
    int64_t *counts;    /* [N], required */
    double *summary;    /* [N][8 + 3 (K-1)], may be NULL */
} hmmsort_spike_fit_out;
int hmmsort_spike_fit(const void *y, int sample_type, int64_t T, const int16_t *x, const int16_t *states, int64_t N,
                      int64_t S, const double *mu, int64_t K, int64_t nchunks, const int64_t *first,
                      const double *mu_track, hmmsort_spike_fit_out *out);
int hmmsort_plan_spike_fit(hmmsort_plan *plan, const double *d_y, const int16_t *d_x, int64_t nchunks,
                           const int64_t *first, const double *mu_track, hmmsort_spike_fit_out *out, void *stream);

/* Widening of raw samples already in device memory into the fp64 signal the plan calls take
 * (src/hmmsort.jl:79-88: `view(data, :, 1)` of the acquisition array, converted to Float64): element i
 * of the output is d_in[i * stride] (stride in elements: 1 for a channel stored contiguously, the
 * channel count for sample-major recordings).  Exact for every source type.  Asynchronous on `stream`.
 * This is the widening alone, for a channel somebody else has cleaned; a raw multi-channel block (drift, mains hum,
 * noise common to the electrodes) goes through hmmsort_preprocess below, which filters and re-references it and
 * widens on the way. */
#define HMMSORT_SAMPLES_I16 0
#define HMMSORT_SAMPLES_I32 1
#define HMMSORT_SAMPLES_F32 2
#define HMMSORT_SAMPLES_F64 3
int hmmsort_samples_to_f64(const void *d_in, int sample_type, int64_t T, int64_t stride, double *d_out,
                           void *stream);

/* Front end for raw recordings (an extension; the reference reads a channel an upstream tool has
 * filtered, src/hmmsort.jl:66-88): a raw block of C channels x T samples, in its own sample type and layout, into
 * the fp64 channel-major array [C][T] that hmmsort_plan_create_batched, hmmsort_fit_channels and
 * hmmsort_seed_templates_device take.  Two stages, all indices 0-based:
 *   1. Zero-phase linear-phase FIR filter per channel.  The filter is given as its half, taps[0..half] with
 *      h[-j] = h[j] = taps[j]; outside [0, T) the signal is mirrored about its end samples without repeating them
 *      (x[-i] = x[i], x[T-1+i] = x[T-1-i]; needs T >= half + 1).  Every multiplication and addition is rounded on its
 *      own (no fused multiply-add), in this order:
 *          acc = taps[0] * x[t];  for j = 1..half ascending:  acc = acc + taps[j] * (x[t-j] + x[t+j]);  f[c][t] = acc
 *      taps == NULL: no filter, f = x exactly (the widening and the channel split alone).
 *   2. Common reference per sample, after the filter.  group[c] >= 0: channels with the same id form a group; < 0:
 *      the channel is filtered only; group == NULL: all channels are group 0.  For a group of G channels
 *      c_0 < c_1 < ... at each sample: HMMSORT_REF_MEDIAN: m = the middle order statistic for odd G, (a + b) * 0.5
 *      for even G with a <= b the two middle ones (exact under ties; a column holding a NaN gives an unspecified m);
 *      HMMSORT_REF_MEAN: s = 0.0; s = s + f[c][t] for c ascending; m = s / G.  out[c][t] = f[c][t] - m.  A group of
 *      one channel comes out as zeros.
 * The result is deterministic to the bit: each output is the work of one thread in a fixed order.
 * Limits, refused before any GPU work with a message that names the argument: HMMSORT_EINVAL for a null in / out,
 * C outside 1..HMMSORT_PRE_MAX_CHANNELS, T outside 1..2^36 or T < half + 1, half outside 0..HMMSORT_PRE_MAX_HALF, an
 * unknown sample type, layout or reference mode, input and output ranges that overlap, a keep entry outside
 * 0..C-1; HMMSORT_EUNSUP for a median group of more than HMMSORT_PRE_MAX_GROUP channels (the mean takes any size).
 * opt == NULL: no filter, no reference.
 * Device form: d_in and d_out are device memory, opt and what it points to host memory (the library uploads the taps
 * and groups itself); writes all C rows (keep is ignored), the reference in place on d_out; its workspace does not
 * depend on T and no widened copy of the block is made; synchronises the stream.  Host form: uploads the block once
 * as it is (2-byte samples stay 2 bytes), runs the device form and downloads the kept rows only; with
 * HMMSORT_REF_NONE only the kept channels are filtered.  No plan is involved. */
#define HMMSORT_LAYOUT_CHANNEL_MAJOR 0 /* in[c * T + t] */
#define HMMSORT_LAYOUT_SAMPLE_MAJOR 1  /* in[t * C + c]: what acquisition systems write */
#define HMMSORT_REF_NONE 0
#define HMMSORT_REF_MEDIAN 1
#define HMMSORT_REF_MEAN 2
#define HMMSORT_PRE_MAX_HALF 4096
#define HMMSORT_PRE_MAX_CHANNELS 1024
#define HMMSORT_PRE_MAX_GROUP 64
typedef struct hmmsort_pre_opt {
    const double *taps;    /* [half + 1] or NULL: no filter */
    int64_t half;          /* P */
    int reference;         /* HMMSORT_REF_* */
    const int32_t *group;  /* [C] or NULL: one group */
    const int32_t *keep;   /* host form only: rows of the result to return, NULL: all C */
    int64_t nkeep;
} hmmsort_pre_opt;
int hmmsort_preprocess(const void *in, int sample_type, int layout, int64_t C, int64_t T,
                       const hmmsort_pre_opt *opt, double *out /* [nkeep or C][T] */);
int hmmsort_preprocess_device(const void *d_in, int sample_type, int layout, int64_t C, int64_t T,
                              const hmmsort_pre_opt *opt, double *d_out /* [C][T] */, void *stream);

/* fit.jl:24-36 on a decoded chunk in device memory.  d_x: the chunk's k states (1 = silent), 1 <= k <= 2^31 - 1.
 * lead  != 0 (the chunk is not the recording's first, fit.jl:24):  l  = 1 + number of leading samples with x > 1,
 *            l = k + 1 when no sample is silent;        lead  == 0: l  = 1.
 * trail != 0 (the chunk does not end the recording, fit.jl:30): kk = 1-based index of the last silent sample,
 *            0 when there is none;                      trail == 0: kk = k.
 * Copies d_x[l-1 .. kk-1] to d_dst[l-1 .. kk-1] (d_dst = where the chunk's first sample belongs in ml_seq);
 * copies nothing when l > kk.  d_lk[0] = l, d_lk[1] = kk (device int64[2]).  Asynchronous on `stream`. */
int hmmsort_chunk_stitch(const int16_t *d_x, int64_t k, int lead, int trail, int16_t *d_dst, int64_t *d_lk,
                         void *stream);

/* Template seed: approximate templates from the recording alone (an extension; the reference starts training from
 * random templates, baumwelch.jl:311-322, and takes sorting templates from a file).  Deterministic, 0-based below:
 *   D = K - 1 snippet samples (row 0 of mu is the silent row and stays 0).
 *   noise scale  sigma_n = (order statistic (T-1)/2 of |y|, exact) / 0.6744897501960817, or opt->sigma when > 0.
 *   v[t] = -y[t], |y[t]| or y[t] for polarity -1, 0, +1.  t is an event iff v[t] > threshold * sigma_n, v[u] < v[t]
 *   for u in [max(0, t-R), t), v[u] <= v[t] for u in (t, min(T-1, t+R)] (a plateau goes to its earliest sample) and
 *   the snippet y[t-align .. t-align+D-1] lies inside the recording.  Events are at least R + 1 apart.
 *   Centres start at the snippets of rank min(E-1, ((2i+1) E) / (2N)) in the order by (v[t], t); then Lloyd
 *   iterations: squared distance accumulated in ascending sample order (multiply and add rounded separately), label
 *   = arg min with ties to the lower i, stop when no label changed or after max_iters assignments; a non-empty
 *   cluster's centre is the mean of its snippets, an empty one keeps its centre.  The sums use no floating-point
 *   atomics and a fixed order: the same input gives the same bits.
 * Outputs (host pointers): mu K x N column-major (rows 1..D = centre i), sigma = sigma_n, counts[i], lp[i] =
 * log(counts[i] / T) (-Inf for an empty cluster), n_events, iters = assignments made, and the first min(n_events, cap)
 * event times (1-based, ascending) and labels (0-based) -- the cap protocol of hmmsort_extract_spiketimes.  No event at
 * all is not an error: mu and counts are zero, lp is -Inf.
 * Limits: 2 <= K <= HMMSORT_SEED_MAX_K, 1 <= N <= HMMSORT_SEED_MAX_N, 1 <= refractory <= HMMSORT_SEED_MAX_R,
 * align < K - 1, K <= T <= 2^40, polarity in -1..1; anything else is HMMSORT_EINVAL before any GPU work.  No plan is
 * involved.  The host form uploads the signal once (int16 samples as they are, widened on the device); sample_type is
 * HMMSORT_SAMPLES_F64 or HMMSORT_SAMPLES_I16.  The device form takes a resident fp64 signal and synchronises the
 * stream. */
#define HMMSORT_SEED_MAX_K 1025
#define HMMSORT_SEED_MAX_N 16
#define HMMSORT_SEED_MAX_R 1024
typedef struct hmmsort_seed_opt {
    double threshold;   /* in units of sigma_n; NaN: 4.0 */
    double sigma;       /* > 0: used as sigma_n; <= 0: the robust estimate */
    int polarity;       /* -1, 0, +1 */
    int64_t align;      /* snippet index of the extremum; < 0: (K - 1) / 3 */
    int64_t refractory; /* R; < 0: K - 1 */
    int64_t max_iters;  /* <= 0: 20 */
} hmmsort_seed_opt;
typedef struct hmmsort_seed_out {
    double *mu;         /* K * N */
    double *sigma;      /* 1 */
    double *lp;         /* N */
    int64_t *counts;    /* N */
    int64_t *n_events;  /* 1, may be NULL */
    int64_t *iters;     /* 1, may be NULL */
    int64_t *times;     /* cap, may be NULL */
    int16_t *labels;    /* cap, may be NULL */
    int64_t cap;
} hmmsort_seed_out;
int hmmsort_seed_templates(const void *y, int sample_type, int64_t T, int64_t N, int64_t K,
                           const hmmsort_seed_opt *opt /* NULL: defaults */, hmmsort_seed_out *out);
int hmmsort_seed_templates_device(const double *d_y, int64_t T, int64_t N, int64_t K, const hmmsort_seed_opt *opt,
                                  hmmsort_seed_out *out, void *stream);

/* Correlograms, refractory violations and coincident spikes of sorted units (an extension): what the
 * spike trains themselves say, beside the per-spike fit above -- the auto-correlogram and ISI violations of a unit, the
 * cross-correlogram of two units, and the share of a unit's spikes another unit also has (a neuron seen on two
 * electrodes comes out of a per-channel sort as two units).  Integers only: the result is a fixed function of the input.
 *   units     u = 0..U-1; unit u has n_u >= 0 spike times t_u[0..n_u), 1-based samples, strictly ascending, each in
 *             1..2^40.
 *   options   (b, H, r, c) = (bin, half_bins, refractory, coincidence), all in samples.
 *   ccg       [U][U][2H] int64: ccg[u][v][k] counts the pairs (i, j) with (u, i) != (v, j), d = t_v[j] - t_u[i],
 *             -H b <= d < H b and k = floor(d / b) + H.  Bin edges are at multiples of b and every bin is half open;
 *             d = 0 between different units lands in bin H; u == v gives the auto-correlogram without the self pair.
 *   viol      [U]: viol[u] = #{ i >= 1 : t_u[i] - t_u[i-1] < r }, consecutive intervals; r = 0 gives 0.
 *   coinc     [U][U]: coinc[u][v] = #{ i : there is j with (v, j) != (u, i) and |t_v[j] - t_u[i]| <= c }; each spike of
 *             u is counted once however many partners it has, so coinc[u][v] / n_u is the share of u's spikes that v
 *             also has.
 *   n         [U]: n[u] = n_u.
 * Outputs are host arrays; any of them except n may be NULL.
 * Refused before any GPU work, HMMSORT_EINVAL (the message names unit and position where one applies): a null required
 * argument, U outside 1..4096, b < 1, H outside 1..2048, H b >= 2^31, r < 0 or c < 0, a negative count, a time outside
 * 1..2^40, a list that is not strictly ascending.  HMMSORT_EUNSUP, naming the number of entries: U U 2H > 2^28.
 * hmmsort_correlograms: host lists, times[u] a host pointer (may be NULL when counts[u] == 0) and counts[u] its
 * length; uploads once, no plan is involved.
 * hmmsort_plan_correlograms: the resident path(s) d_x of a plan ([C][T] for a batched plan).  Units are u = ch N + a;
 * the events are exactly those of hmmsort_plan_extract_spiketimes under the plan's current model, compacted on the
 * device, and never come to the host -- only the counts do.  Pairs across channels are included.  Any engine.
 * Synchronises the stream.  Channels with different models, lengths or devices go through the host form. */
typedef struct hmmsort_ccg_opt {
    int64_t bin;          /* b: bin width */
    int64_t half_bins;    /* H: bins on each side of lag 0 */
    int64_t refractory;   /* r */
    int64_t coincidence;  /* c */
} hmmsort_ccg_opt;
typedef struct hmmsort_ccg_out {
    int64_t *ccg;     /* [U][U][2H], may be NULL */
    int64_t *viol;    /* [U], may be NULL */
    int64_t *coinc;   /* [U][U], may be NULL */
    int64_t *n;       /* [U], required */
} hmmsort_ccg_out;
int hmmsort_correlograms(int64_t U, const int64_t *const *times, const int64_t *counts, const hmmsort_ccg_opt *opt,
                         hmmsort_ccg_out *out);
int hmmsort_plan_correlograms(hmmsort_plan *plan, const int16_t *d_x, const hmmsort_ccg_opt *opt, hmmsort_ccg_out *out,
                              void *stream);

/* Footprints: the spike-triggered sum of every unit on every channel of a block (an extension).  A
 * per-channel sort looks at a unit on its own channel only; the footprint says on which channel the unit is largest,
 * whether two coincident units have the same shape across the channels, and where along a probe the unit sits.  All
 * indices 0-based unless stated.
 *   block     y[C][T], channel-major, fp64 (the host form also takes int16, widened exactly on the device).
 *   units     u = 0..U-1; unit u has n_u >= 0 spike times, 1-based samples, strictly ascending, each in 1..2^40 (the
 *             lists of hmmsort_correlograms).
 *   options   pre >= 0, W >= 1, M and chan: an optional int32 table [U][M] of block channels per unit; an entry in
 *             0..C-1 may repeat and may come in any order, -1 marks an empty slot.  chan == NULL: M = C (the M given is
 *             ignored) and slot m is channel m for every unit.
 *   snippet   of a spike at time t on channel c: s[k] = y[c][t - 1 - pre + k], k = 0..W-1.  The spike is used iff
 *             t - 1 - pre >= 0 and t - 1 - pre + W <= T, for all channels alike; a time beyond T is unused, no error.
 *   outputs   host arrays sum[U][M][W], sumsq[U][M][W], nused[U] (used spikes), n[U] = n_u; sum, sumsq and nused may
 *             each be NULL, n is required.  An empty slot and a unit without a used spike give zeros.
 *   order     no floating-point atomics; the same input gives the same bits.  The list of a unit is cut into blocks of
 *             256 consecutive list entries (the constant of hmmsort_spike_fit's summary), whichever of them are used.
 *             Within a block, per (slot, k), a serial fold from 0.0 over the used spikes in ascending order:
 *             ps = ps + s; pq = pq + s * s, the product rounded on its own (never fused).  The block partials are then
 *             folded serially from 0.0 in block order; a block without a used spike contributes its 0.0.
 * Refused before any GPU work, HMMSORT_EINVAL with a message that names the argument (and unit and position where one
 * applies): a null required argument, C outside 1..HMMSORT_PRE_MAX_CHANNELS, T outside 1..2^36, U outside
 * 1..HMMSORT_FP_MAX_UNITS, W outside 1..HMMSORT_FP_MAX_W, pre outside 0..2^20, M outside 1..HMMSORT_FP_MAX_SLOTS, a chan
 * entry outside -1..C-1, a negative count, a time outside 1..2^40, a list that is not strictly ascending, a sample type
 * other than F64 / I16.  HMMSORT_EUNSUP, naming the number of entries: U M W > 2^28.  W > T is legal: every spike is
 * unused.  A refused call leaves every output array untouched.
 * hmmsort_footprints: host buffers, no plan; uploads the block once (2-byte samples stay 2 bytes on the way).
 * hmmsort_footprints_device: d_y the resident fp64 block, the lists concatenated in device memory behind U + 1 host
 * offsets (offs[0] >= 0, ascending); the times themselves are not checked -- a time whose window leaves the block is
 * unused whatever it is, so nothing outside d_y[0 .. C T) and d_times[offs[0] .. offs[U]) is read.  Synchronises the
 * stream.
 * hmmsort_plan_footprints: units u = ch N + a from the resident path(s) d_x of a plan, exactly the events of
 * hmmsort_plan_extract_spiketimes under the plan's current model, compacted on the device (they never come to the
 * host); d_block any resident [Cb][T] fp64 block of the plan's T, Cb need not be the plan's channel count.  Any
 * engine.  Synchronises the stream. */
#define HMMSORT_FP_MAX_UNITS 4096
#define HMMSORT_FP_MAX_W 1024
#define HMMSORT_FP_MAX_SLOTS 1024
typedef struct hmmsort_fp_opt {
    int64_t pre;          /* samples of the window before the spike time */
    int64_t W;            /* window length */
    int64_t M;            /* slots per unit (chan != NULL) */
    const int32_t *chan;  /* [U][M] host table or NULL: all C channels in order */
} hmmsort_fp_opt;
typedef struct hmmsort_fp_out {
    double *sum;      /* [U][M][W], may be NULL */
    double *sumsq;    /* [U][M][W], may be NULL */
    int64_t *nused;   /* [U], may be NULL */
    int64_t *n;       /* [U], required */
} hmmsort_fp_out;
int hmmsort_footprints(const void *y, int sample_type, int64_t C, int64_t T, int64_t U, const int64_t *const *times,
                       const int64_t *counts, const hmmsort_fp_opt *opt, hmmsort_fp_out *out);
int hmmsort_footprints_device(const double *d_y, int64_t C, int64_t T, int64_t U, const int64_t *d_times,
                              const int64_t *offs, const hmmsort_fp_opt *opt, hmmsort_fp_out *out, void *stream);
int hmmsort_plan_footprints(hmmsort_plan *plan, const int16_t *d_x, const double *d_block, int64_t Cb,
                            const hmmsort_fp_opt *opt, hmmsort_fp_out *out, void *stream);

/* Waveform features and cluster isolation (an extension): one feature row per spike, the moments of the
 * rows per unit, and from rows, unit means and inverse covariances the figures that say whether a unit is separated
 * from the other units and the noise in waveform space (isolation distance and L-ratio, Schmitzer-Torbert et al.
 * 2005).  The small linear algebra between the calls (PCA, the covariance inverse) is the host's: api.pca_basis,
 * api.cluster_isolation.  No floating-point atomics, no fused multiply-add, no matrix-core instructions: every result
 * but lpair is a fixed function of the input that tests/feature_model.py reproduces bit for bit.  All indices 0-based
 * unless stated.
 *
 * 1. hmmsort_snippet_features.  Block, units, pre, W, the snippet s_m[k] = y[chan[m]][t - 1 - pre + k] and the rule
 *    "used iff the window lies inside the block" are those of hmmsort_footprints.
 *   options   chan: ONE int32 row [M] for all units (entries in 0..C-1, repeats allowed; NULL: M = C, all channels in
 *             order, the M given is ignored).  basis [M][P][W] and centre [M][W], host doubles; centre NULL means
 *             zeros; basis NULL: P := W (the P given is only checked to be >= 1).  moments: 0, 1 or 2.
 *   rows      entry e of unit u is row r = offs[u] - offs[0] + e (host form: offs from the counts); n_total rows of
 *             F features.  Without a basis F = M W and f[r][m W + k] = s_m[k] - centre[m][k]; with centre NULL that
 *             is the snippet itself, bit for bit.  With a basis F = M P and f[r][m P + p] = acc, where acc = +0.0 and,
 *             for k ascending, acc = acc + basis[m][p][k] * (s_m[k] - centre[m][k]): the subtraction, the product
 *             and the sum each rounded on their own.  An unused entry's row is +0.0 and its used byte 0.
 *   outputs   feat[n_total][F] and used[n_total] (bytes), each may be NULL: host arrays in the host form, device
 *             memory in the device and plan forms.  Host arrays n[U] (required), nused[U] (may be NULL), and the
 *             moments the mode asks for (required then).
 *   moments   1: per unit and slot b1[U][M][P], b2[U][M][P][P]; 2: per unit g1[U][F], g2[U][F][F].  A unit's list is
 *             cut into tiles of 256 consecutive list entries, used or not.  Within a tile a serial fold from +0.0
 *             over the used entries in ascending order: p1_a = p1_a + f_a; p2_ab = p2_ab + f_a * f_b, the product
 *             rounded on its own.  The tile partials are folded serially from +0.0 in tile order.  b >= a is computed
 *             and mirrored.
 *   refused   before any GPU work, every output untouched, the message names the argument.  HMMSORT_EINVAL: what
 *             hmmsort_footprints refuses (a chan entry must be in 0..C-1 here), moments outside 0..2 or without its
 *             output arrays, P < 1, P > W with a basis, a basis or centre entry that is not finite.  HMMSORT_EUNSUP,
 *             naming the numbers: moments = 1 with P > HMMSORT_FEAT_MAX_P1, moments = 2 with F > HMMSORT_FEAT_MAX_F2,
 *             n_total F > 2^31, U M P P or U F F above 2^26.  (The plan form learns n_total from the compaction, so
 *             it refuses n_total F after that.)  W > T is legal: every row is unused and nothing is read.
 *   forms     hmmsort_snippet_features: host buffers; uploads the block once (2-byte samples stay 2 bytes on the way).
 *             _device: d_y, d_times and host offs as hmmsort_footprints_device; synchronises the stream.
 *             hmmsort_plan_snippet_features: units u = ch N + a of the plan's resident path(s) as
 *             hmmsort_plan_footprints finds them, d_block [Cb][T]; cap_rows is what d_feat and d_used can hold in
 *             rows: cap_rows < n_total writes no row and no byte and is no error (n[U] says how many are needed; a
 *             first call with feat == NULL is the usual moments pass).  Synchronises the stream.
 *
 * 2. hmmsort_cluster_isolation.  feat[n][F] rows in unit order behind host offs[U + 1] (n = offs[U] - offs[0]), used[n]
 *    bytes or NULL for all used, host mu[U][F] and Vinv[U][F][F] (need not be symmetric); F in
 *    1..HMMSORT_FEAT_MAX_F2, U in 1..HMMSORT_FP_MAX_UNITS.  A unit whose Vinv[u][0][0] is NaN is not scored: its
 *    outputs are NaN / -1 (the rest of its mu and Vinv is not read), and its spikes still count as non-members of
 *    the other units.
 *   distance  for a scored unit u and a used row r: d_b = f[r][b] - mu[u][b]; q = +0.0; for a ascending: rr = +0.0; for
 *             b ascending rr = rr + Vinv[u][a][b] * d_b; then q = q + d_a * rr; every product and sum rounded on its
 *             own.  d2[u][r] = q if q > 0, else +0.0.
 *   outputs   host arrays, each may be NULL.  iso_d2[U]: with n_u the used members and n_o the used non-members, if
 *             n_u >= 1 and n_o >= n_u the exact order statistic of rank n_u - 1 (0-based) of d2[u][.] over the used
 *             non-member rows, else NaN.  closer[U][U] int64: the count of {r in v, used: d2[u][r] < d2[v][r]},
 *             strict; 0 on the diagonal, -1 when either unit is not scored.  lpair[U][U]: the sum over the used r in
 *             v of Q_F(d2[u][r]), folded by tiles of 256 list entries of v, serially within a tile and across tiles;
 *             0 on the diagonal, NaN for a u that is not scored.  Q_F is the chi-square survival function: with
 *             h = x / 2, e = exp(-h); e == 0 gives 0; even F: e * sum_{j < F/2} t_j, t_0 = 1, t_j = t_{j-1} * h / j;
 *             odd F: erfc(sqrt(h)) + e * sqrt(h) * (2 / sqrt(pi)) * sum_{j <= (F-3)/2} t_j, t_0 = 1,
 *             t_j = t_{j-1} * h / (j + 0.5), no second term for F = 1.  lpair follows the device's exp, erfc and sqrt
 *             and is therefore not bit-exact against another library (DESIGN 3.17 has the measured difference).
 *   refused   before any GPU work: HMMSORT_EINVAL for a null required argument, F or U outside their ranges,
 *             descending offs, n != offs[U] - offs[0], any other non-finite mu / Vinv entry of a scored unit;
 *             HMMSORT_EUNSUP for U n > 2^30.
 *   forms     hmmsort_cluster_isolation: host feat / used.  _device: device feat / used; synchronises the stream. */
#define HMMSORT_FEAT_MAX_P1 128
#define HMMSORT_FEAT_MAX_F2 64
typedef struct hmmsort_feat_opt {
    int64_t pre;           /* samples of the window before the spike time */
    int64_t W;             /* window length */
    int64_t M;             /* slots (chan != NULL) */
    const int32_t *chan;   /* [M] host row or NULL: all C channels in order */
    int64_t P;             /* components per slot (basis != NULL) */
    const double *basis;   /* [M][P][W] host or NULL */
    const double *centre;  /* [M][W] host or NULL: zeros */
    int64_t moments;       /* 0: none, 1: per unit and slot, 2: per unit */
} hmmsort_feat_opt;
typedef struct hmmsort_feat_out {
    double *feat;          /* [n_total][F], may be NULL; device memory in the device and plan forms */
    unsigned char *used;   /* [n_total], may be NULL; likewise */
    int64_t cap_rows;      /* plan form: rows feat and used can hold */
    int64_t *n;            /* [U], required */
    int64_t *nused;        /* [U], may be NULL */
    double *b1, *b2;       /* moments = 1: [U][M][P], [U][M][P][P] */
    double *g1, *g2;       /* moments = 2: [U][F], [U][F][F] */
} hmmsort_feat_out;
int hmmsort_snippet_features(const void *y, int sample_type, int64_t C, int64_t T, int64_t U,
                             const int64_t *const *times, const int64_t *counts, const hmmsort_feat_opt *opt,
                             hmmsort_feat_out *out);
int hmmsort_snippet_features_device(const double *d_y, int64_t C, int64_t T, int64_t U, const int64_t *d_times,
                                    const int64_t *offs, const hmmsort_feat_opt *opt, hmmsort_feat_out *out,
                                    void *stream);
int hmmsort_plan_snippet_features(hmmsort_plan *plan, const int16_t *d_x, const double *d_block, int64_t Cb,
                                  const hmmsort_feat_opt *opt, hmmsort_feat_out *out, void *stream);
typedef struct hmmsort_iso_out {
    double *iso_d2;    /* [U], may be NULL */
    int64_t *closer;   /* [U][U], may be NULL */
    double *lpair;     /* [U][U], may be NULL */
} hmmsort_iso_out;
int hmmsort_cluster_isolation(const double *feat, int64_t n, int64_t F, int64_t U, const int64_t *offs,
                              const unsigned char *used, const double *mu, const double *Vinv, hmmsort_iso_out *out);
int hmmsort_cluster_isolation_device(const double *d_feat, int64_t n, int64_t F, int64_t U, const int64_t *offs,
                                     const unsigned char *d_used, const double *mu, const double *Vinv,
                                     hmmsort_iso_out *out, void *stream);

/* Unit stability over time (an extension): was the unit there the whole time?  Spike counts per unit and
 * time bin, and of one fp64 value per spike (its amplitude, usually) exact order statistics, sums and a histogram, per
 * unit and time bin and per unit over the whole recording -- what firing rate per bin, presence ratio, amplitude drift
 * and amplitude cutoff rest on (api.UnitStability has those finishers).  Every result is a fixed function of the input
 * that tests/stability_model.py reproduces bit for bit: no interpolation, no fused multiply-add, no floating-point
 * atomics, no matrix-core instructions.  All indices 0-based except spike times.
 *   units     u = 0..U-1; unit u has n_u >= 0 spike times, 1-based samples, strictly ascending, each in 1..T, and, when
 *             values are given, one fp64 value per spike.  A NaN value means "no value": it is not valid and takes no
 *             part in order statistics, sums or histogram.  values == NULL: only n and count are written.
 *   options   T the recording length; bin >= 1 samples per time bin, B = ceil(T / bin), bin b holds the times with
 *             (t - 1) / bin == b in integer division, the last bin may be short.  nq <= HMMSORT_STAB_MAX_Q quantiles
 *             q_num[k] / q_den with 0 <= q_num[k] <= q_den <= HMMSORT_STAB_MAX_QDEN.  A histogram of HB >= 0 bins.
 *   segment   (u, b): the spikes of unit u in bin b, a contiguous range of its list; (u): all of them.
 *   order     of values: that of the bit patterns mapped monotonically, -Inf < ... < -0.0 < +0.0 < ... < +Inf.
 *   quantile  k of a segment with m valid values: the order statistic of 0-based rank floor(q_num[k] (m - 1) / q_den),
 *             in 64-bit integers (q_num <= 2^20 and m < 2^31, so the product stays below 2^51).  The result is one of
 *             the inputs, bit for bit; ties between equal patterns cannot change it.  NaN when m == 0.
 *   sums      sum and sumsq of a segment (u, b): its valid values in ascending event order are cut into tiles of 256;
 *             within a tile a serial fold from +0.0: ps = ps + v; pq = pq + v * v, the square rounded on its own; the
 *             tile partials are folded serially from +0.0 in tile order.  usum[u] / usumsq[u] fold sum[u][.] /
 *             sumsq[u][.] serially from +0.0 in bin order (the bin sums, not the events again).
 *   histogram of unit u over its valid values: p = (v - hist_lo) * hist_scale, the subtraction and the product rounded
 *             separately; p < 0 counts in under[u], p >= HB in over[u], else hist[u][floor(p)].
 *   outputs   host arrays, any of them except n may be NULL: n[U]; count[U][B], valid[U][B] int64; quant[U][B][nq];
 *             sum[U][B], sumsq[U][B]; uvalid[U]; uquant[U][nq]; umin[U], umax[U] (ranks 0 and m - 1, NaN when there is
 *             no valid value); usum[U], usumsq[U]; hist[U][HB], under[U], over[U] int64.
 *   refused   before any GPU work, every output untouched, the message names the argument.  HMMSORT_EINVAL: a null
 *             required pointer, U outside 1..HMMSORT_STAB_MAX_UNITS, T outside 1..2^40, bin < 1, nq outside
 *             0..HMMSORT_STAB_MAX_Q, q_den outside 1..HMMSORT_STAB_MAX_QDEN, a q_num outside 0..q_den, HB outside
 *             0..HMMSORT_STAB_MAX_HIST, with HB > 0 a hist_scale that is not finite and positive or a hist_lo that is
 *             not finite, a negative count, a time outside 1..T, a list that is not strictly ascending, a unit with
 *             spikes and a null values[u] beside a non-null values.  HMMSORT_EUNSUP, naming the number: B or U B above
 *             HMMSORT_STAB_MAX_BINS (so quant stays below 2^28 entries), 2^31 spikes or more in all.
 *   forms     hmmsort_unit_stability: host lists, times[u] and values[u] host pointers (NULL allowed for an empty
 *             unit); uploads once, no plan is involved.
 *             hmmsort_unit_stability_device: d_times and d_values (or NULL) hold the U lists one after the other in
 *             device memory behind U + 1 host offsets (offs[0] >= 0, ascending), as hmmsort_footprints_device takes
 *             them.  The times cannot be checked before the GPU runs: a time below 1 counts in bin 0, one beyond T in
 *             the last bin, and a list whose bin boundaries step back is refused after the search (HMMSORT_EINVAL, n
 *             already written); nothing outside [offs[0], offs[U]) is read.  Synchronises the stream.
 *             hmmsort_plan_unit_stability: units u = ch N + a of the resident path(s) d_x of a plan ([C][T] for a
 *             batched plan), exactly the events of hmmsort_plan_extract_spiketimes; the value of an event is the amp of
 *             hmmsort_plan_spike_fit under the plan's current model (no track), computed by the same code.  opt->T must
 *             be the plan's T.  Neither events nor amplitudes come to the host.  Any engine.  Synchronises the
 *             stream. */
#define HMMSORT_STAB_MAX_UNITS 4096
#define HMMSORT_STAB_MAX_Q 8
#define HMMSORT_STAB_MAX_QDEN (1ll << 20)
#define HMMSORT_STAB_MAX_HIST 4096
#define HMMSORT_STAB_MAX_BINS (1ll << 24)
typedef struct hmmsort_stab_opt {
    int64_t T;            /* recording length in samples */
    int64_t bin;          /* samples per time bin */
    int64_t nq;           /* quantiles */
    int64_t q_num[HMMSORT_STAB_MAX_Q];
    int64_t q_den;
    int64_t HB;           /* histogram bins, 0: none */
    double hist_lo;       /* left edge of histogram bin 0 */
    double hist_scale;    /* 1 / bin width */
} hmmsort_stab_opt;
typedef struct hmmsort_stab_out {
    int64_t *n;           /* [U], required */
    int64_t *count;       /* [U][B] */
    int64_t *valid;       /* [U][B] */
    double *quant;        /* [U][B][nq] */
    double *sum, *sumsq;  /* [U][B] */
    int64_t *uvalid;      /* [U] */
    double *uquant;       /* [U][nq] */
    double *umin, *umax;  /* [U] */
    double *usum, *usumsq; /* [U] */
    int64_t *hist;        /* [U][HB] */
    int64_t *under, *over; /* [U] */
} hmmsort_stab_out;
int hmmsort_unit_stability(int64_t U, const int64_t *const *times, const double *const *values /* may be NULL */,
                           const int64_t *counts, const hmmsort_stab_opt *opt, hmmsort_stab_out *out);
int hmmsort_unit_stability_device(int64_t U, const int64_t *d_times, const double *d_values /* may be NULL */,
                                  const int64_t *offs, const hmmsort_stab_opt *opt, hmmsort_stab_out *out,
                                  void *stream);
int hmmsort_plan_unit_stability(hmmsort_plan *plan, const double *d_y, const int16_t *d_x, const hmmsort_stab_opt *opt,
                                hmmsort_stab_out *out, void *stream);

/* Spatial whitening (an extension): the noise covariance of the quiet samples of a block, and a mix of
 * its channels, on the fp64 channel-major block [C][T] that hmmsort_preprocess_device writes.  The C x C matrix itself
 * (ZCA, global or local) is the host's work: api.whitening_matrix.  All indices 0-based.  No floating-point atomics,
 * no fused multiply-add and no matrix-core instructions: every result is a fixed function of the input that
 * tests/whiten_model.py reproduces bit for bit.
 *   1. noise scale   sigma[c] = (order statistic (T-1)/2 of |y[c][.]|, exact) / 0.6744897501960817, the rule of
 *                    hmmsort_seed_templates; all channels in one grid.  A row that holds a NaN gives an unspecified
 *                    sigma.
 *   2. quiet mask    thr[c] = threshold * sigma[c] (threshold NaN: 4.0), or the caller's thr[C], and then stage 1 is
 *                    skipped.  loud[t] iff some channel has !(|y[c][t]| <= thr[c]), so a NaN or Inf sample is loud.
 *                    quiet[t] iff no u in [max(0, t - guard), min(T - 1, t + guard)] is loud (guard < 0: 30).
 *                    n_quiet counts the quiet samples; d_quiet, when given, receives quiet[t] as 0 / 1 bytes.
 *   3. sums          s1[C], s2[C][C] over the quiet samples, raw (the host divides).  The block is cut into tiles of
 *                    256 consecutive samples, quiet or not.  Within a tile every entry is a serial fold from +0.0 over
 *                    the tile's quiet samples in ascending t: p1_i = p1_i + y_i; p2_ij = p2_ij + y_i * y_j, the product
 *                    rounded on its own.  A sample that is not quiet contributes nothing (a NaN in it never enters).
 *                    The tile partials are folded serially from +0.0 in tile order.  j >= i is computed and mirrored.
 *                    n_quiet == 0 is no error: the sums are zeros.
 *   4. channel mix   out[r][t]: acc = +0.0; for m = 0..M-1 ascending with nbr[r][m] >= 0:
 *                    acc = acc + w[r][m] * in[nbr[r][m]][t], multiply and add rounded separately.  nbr int32 [R][M] and
 *                    w double [R][M] are host memory (the library uploads them); -1 is an empty slot, repeats and any
 *                    order are allowed, a row of empty slots comes out as zeros.  Global whitening is R = M = C with
 *                    nbr[r] = 0..C-1; local whitening and any re-montage use the same call.  d_out == d_in exactly
 *                    with R == C is allowed (a workgroup stages all rows of its samples before it writes any).
 * Refused before any GPU work, HMMSORT_EINVAL with a message that names the argument, every output untouched: a null
 * required pointer, C, R or M outside 1..HMMSORT_WHITEN_MAX_CHANNELS, T outside 1..2^36, guard above
 * HMMSORT_WHITEN_MAX_GUARD, a thr[c] that is not positive (NaN included), a negative threshold, an nbr entry outside
 * -1..C-1, input and output ranges that overlap in part, in place with R != C, d_quiet in the host form.
 * The device forms synchronise the stream; their workspace does not depend on T except the mask (T bytes), the mask's
 * per-tile records and a bounded buffer of tile partials.  The host forms upload the block once and run the device
 * forms.  No plan is involved. */
#define HMMSORT_WHITEN_MAX_CHANNELS 1024
#define HMMSORT_WHITEN_MAX_GUARD 65536
typedef struct hmmsort_noise_opt {
    double threshold;   /* in units of sigma[c]; NaN: 4.0 */
    const double *thr;  /* [C] absolute thresholds or NULL */
    int64_t guard;      /* samples either side of a loud one; < 0: 30 */
} hmmsort_noise_opt;
typedef struct hmmsort_noise_out {
    double *sigma;     /* [C], written only when thr == NULL; may be NULL */
    int64_t *n_quiet;  /* 1 */
    double *s1;        /* [C] */
    double *s2;        /* [C*C] */
    uint8_t *d_quiet;  /* device [T], may be NULL */
} hmmsort_noise_out;
int hmmsort_noise_scale_device(const double *d_y, int64_t C, int64_t T, double *sigma /* host [C] */, void *stream);
int hmmsort_noise_cov_device(const double *d_y, int64_t C, int64_t T, const hmmsort_noise_opt *opt /* NULL: defaults */,
                             hmmsort_noise_out *out, void *stream);
int hmmsort_noise_cov(const double *y /* host [C][T] */, int64_t C, int64_t T, const hmmsort_noise_opt *opt,
                      hmmsort_noise_out *out /* d_quiet must be NULL */);
int hmmsort_channel_mix_device(const double *d_in, int64_t C, int64_t T, int64_t R, int64_t M, const int32_t *nbr,
                               const double *w, double *d_out /* [R][T] */, void *stream);
int hmmsort_channel_mix(const double *in, int64_t C, int64_t T, int64_t R, int64_t M, const int32_t *nbr,
                        const double *w, double *out);

/* Per-kernel timing of the ring engine with HIP events recorded on the caller's stream (used by
 * bench.py for the roofline line).  hmmsort_plan_profile(plan, 1) switches bracketing on;
 * hmmsort_plan_profile_read synchronises the stream and returns, per kernel name, the total
 * milliseconds and the number of launches since the previous read.  `names` receives the kernel
 * names joined by '\n'. */
int hmmsort_plan_profile(hmmsort_plan *plan, int enable);
int hmmsort_plan_profile_read(hmmsort_plan *plan, void *stream, char *names, int64_t names_cap,
                              double *ms, int64_t *calls, int64_t cap, int64_t *n_out);

#ifdef __cplusplus
}
#endif
#endif /* HMMSORT_H */

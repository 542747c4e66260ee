/* hml.h - C ABI of the MI355X-native HaMMLET hot path (libhammlet_hip.so).
 *
 * The reference (wiedenhoeft/HaMMLET) is one header-only C++ program with no FFI seam; the
 * types it instantiates in src/main.cpp:338-362,437,444 are what a drop-in has to stand behind.
 * Every entry point below names the reference interface it replaces (file:line relative to the
 * reference's repository root).  INTEGRATION.md shows the reference-side binding.
 *
 * Conventions: plain pointers and sizes only; every function returns 0 on success and a non-zero
 * code on failure, with the message available from hml_last_error() (the text of the
 * std::runtime_error the reference would have thrown, where one exists).  A context owns all
 * device memory of one chain on one GPU and is not thread-safe (the reference is single-threaded
 * with one shared RNG, src/main.cpp:108).  All work is enqueued on the context's HIP stream;
 * functions that return data to the host synchronise that stream.
 */
#ifndef HML_H
#define HML_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hml_ctx hml_ctx;

/* sampling methods of hml_iterate (src/main.cpp:432-445: "F" and "M" scheme tokens) */
#define HML_METHOD_FB 'F'
#define HML_METHOD_MIXTURE 'M'

/* error codes */
#define HML_OK 0
#define HML_ERR_ARG 1      /* invalid argument / call order                                  */
#define HML_ERR_HIP 2      /* HIP runtime failure                                            */
#define HML_ERR_MODEL 3    /* a model invariant the reference enforces by throwing was hit   */

const char* hml_last_error(void);

/* Library/ABI version and the GPU architecture the kernels were compiled for ("gfx950"). */
uint32_t hml_abi_version(void);
const char* hml_device_arch(void);
/* number of GPUs this process can use (hipGetDeviceCount) */
int hml_device_count(int* n);

/* rng_t RNG(seed) (src/main.cpp:107-108) + one chain's device state.  `stream` may be NULL
 * (a private stream is created) or a hipStream_t owned by the caller. */
int hml_create(hml_ctx** out, int device, uint64_t seed, uint32_t chain_id, void* stream);
void hml_destroy(hml_ctx* ctx);

/* MaxletTransform + noise estimate + HaarBreakpointWeights + Statistics<IntegralArray,Normal> +
 * Blocks<BreakpointArray> constructors (src/wavelet.hpp:68-188, src/main.cpp:303-318,340-341,
 * src/Statistics/IntegralArray.hpp:136-191, src/Blocks/BreakpointArray.hpp:130-184).
 * hml_load_observations: n_values = T host floats - T * D after hml_set_dimensions(D, .), the D values of a position one
 * after the other.  hml_load_observations_device: T device floats (univariate; sigma-hat is then computed from a host copy
 * made internally). */
int hml_load_observations(hml_ctx* ctx, const float* x, uint64_t n_values);
int hml_load_observations_device(hml_ctx* ctx, const void* x_dev, uint64_t T);

/* A further chain over the SAME observations on the same GPU (chains outnumbering GPUs: `hammlet -chains N`, several
 * chains per rank): `ctx` shares `source`'s read-only construction - breakpoint weights and their summary, maxlet
 * coefficients, integral arrays; reference counted, freed with the last context - instead of uploading and building a copy
 * of its own; block structure, sweep buffers, model and marginals stay per chain.  Chains of one run read the same trace
 * and their block sets are nested by threshold, so their gathers then hit the same cache lines (hml_iterate_many batches
 * such chains through ONE block kernel).  Replaces hml_load_observations for `ctx`; dimensions (hml_set_dimensions) are taken
 * from the source.  hml_scale_weights / hml_set_weights are refused while the weights are shared: apply them to the source
 * first.  The reference builds the construction once per process for its single chain (src/main.cpp:286-343). */
int hml_attach_observations(hml_ctx* ctx, hml_ctx* source);

/* Text input: the values that `while ( input >> v )` extracts from a whitespace-separated decimal stream
 * (src/wavelet.hpp:131, called from src/main.cpp:266-291), converted on the GPU chunk by chunk.  The result is
 * bit-identical to the stream extraction, including where it stops: tokens the device cannot decide with proof
 * (more than 19 significant digits, ties, sub-normal or overflowing values, anything that is not one plain decimal
 * number from blank to blank) are re-read by the host with that same extraction.
 *   hml_text_open(&r, device, chunk_bytes);          (chunk_bytes 0 = 64 MiB staging)
 *   loop: hml_text_buffer(r, &buf, &cap); n = read(fd, buf, cap); hml_text_commit(r, n);   (or hml_text_feed)
 *   hml_text_finish(r, &n_values, &stopped);  hml_text_values(r, out);  hml_text_close(r);
 * `stopped` = 1 if an extraction failed before the end of the text (the reference silently stops reading there). */
typedef struct hml_text hml_text;
int hml_text_open(hml_text** out, int device, uint64_t chunk_bytes);
void hml_text_close(hml_text* reader);
int hml_text_buffer(hml_text* reader, char** buf, uint64_t* capacity);
int hml_text_commit(hml_text* reader, uint64_t nbytes);
int hml_text_feed(hml_text* reader, const char* bytes, uint64_t nbytes);
/* optional: an upper estimate of the number of values (the reference's reserveT, src/wavelet.hpp:103,123-124) */
int hml_text_reserve(hml_text* reader, uint64_t n_values);
int hml_text_finish(hml_text* reader, uint64_t* n_values, int* stopped);
int hml_text_values(hml_text* reader, float* out /* n_values */);
/* bytes consumed, tokens resolved by the host, chunks that went through the host extraction entirely */
int hml_text_counters(hml_text* reader, uint64_t* bytes_in, uint64_t* irregular_tokens, uint64_t* host_chunks);

/* "-s C P D" (src/main.cpp:114-137, src/Mapping.hpp:53-137): D data dimensions whose values follow each other in the
 * observation stream and P emission parameters shared by K = P^D states (state s uses parameter (s / P^d) % P for
 * dimension d).  Call before hml_load_observations (which then takes T * D values); hml_set_model's K must be P^D;
 * hml_get_theta / hml_set_parameters carry P (mean, variance) pairs.  P = 0 here: taken from hml_set_model's K.
 * Default: D = 1, P = K. */
int hml_set_dimensions(hml_ctx* ctx, int D, int P);
int hml_get_dimensions(hml_ctx* ctx, int* D, int* P);

/* Blocks<BreakpointArray>(vector<real_t>& weights) (src/Blocks/BreakpointArray.hpp:130-184, src/main.cpp:341): replaces
 * the breakpoint weights the device computed by the caller's T host values - for drivers that, like the reference's,
 * hold the weights on the host between HaarBreakpointWeights and the Blocks constructor (and may have changed them). */
int hml_set_weights(hml_ctx* ctx, const float* w, uint64_t T);

/* stdEstimate of src/main.cpp:303-311 */
int hml_noise_sigma(hml_ctx* ctx, double* sigma);

/* `for (auto& w : inputValues) w *= weightMultiplier` (src/main.cpp:332-334) */
int hml_scale_weights(hml_ctx* ctx, float multiplier);

/* autoPrior (src/AutoPriors.hpp:86-110, :18-80): s2 = VAR and p = P of "-e normal VAR P".
 * out4 = {alpha, beta, mu0, nu}.  Leaves the universal threshold as the current threshold. */
int hml_autoprior(hml_ctx* ctx, float s2, float p, float out4[4]);

/* Mapping/Transitions/Initial/TransitionHyperParam/InitialHyperParam/ThetaHyperParam/Theta
 * construction (src/main.cpp:133-166,354-362).  nig4 = {alpha,beta,mu0,nu} shared by all K
 * emission parameters; a_off/a_diag = "-t" tokens; pi_alpha = "-I"; self_trans = !"-S".
 * Like Theta's constructor (src/Theta.hpp:126-127) this draws theta once from the prior.
 * K: 2 .. 64 (the reference takes any -s K, src/main.cpp:112-137).  Up to 16 states the sweep runs kernels instantiated for that
 * number of states; from 17 on the number of states is a run-time value and a state is a lane (hml_k_wide.h) - the same chain
 * semantics (Philox addresses, hml_math.h, the count tree), about three times the time per block of a 16-state model. */
int hml_set_model(hml_ctx* ctx, int K, const float nig4[4], float a_off, float a_diag, float pi_alpha,
                  int self_trans);

/* useSelfTransitions, the last argument of StateSequence::sample / sampleHMM (src/StateSequence.hpp:64, src/HMM.hpp:75):
 * a driver in the reference's shape only states it when it samples, after the model objects exist. */
int hml_set_self_transitions(hml_ctx* ctx, int on);

/* theta.sample(tau_theta); pi.sample(tau_pi); A.sample(tau_A) from the priors
 * (src/main.cpp:393-401, and again after a "P" token). */
int hml_sample_prior(hml_ctx* ctx);

/* "S" token: y.createBlocks(theta); dynamic = false (src/main.cpp:407-414).
 * "D" token: dynamic = true (src/main.cpp:415-421). */
int hml_set_static_blocks(hml_ctx* ctx);
int hml_set_dynamic(hml_ctx* ctx, int on);

/* Emissions::createBlocks(real_t) (src/Emissions.hpp:49-51) + a full enumeration with block
 * statistics (Emissions::next, src/Emissions.hpp:88-95): parity probe for block structures. */
int hml_create_blocks(hml_ctx* ctx, float threshold);

/* sampleHMM (src/HMM.hpp:60-125) with StateSequence<ForwardBackward> or <Mixture>
 * (src/StateSequence/ForwardBackward.hpp:16-213, Mixture.hpp:31-144): `iterations` Gibbs sweeps,
 * recording when thinning > 0 && (i+1) % thinning == 0.  Device-resident; returns after the
 * sweeps are enqueued unless per-sweep side files were requested with hml_set_recording. */
int hml_iterate(hml_ctx* ctx, char method, uint64_t iterations, uint64_t thinning);

/* Records::setRecord* (src/Records.hpp:121-144).  marginals: accumulate state marginals on the
 * device.  The other four make hml_iterate call `cb` after every recorded sweep (with the stream
 * synchronised) so the host can pull blocks/states/theta and append its files
 * (src/Records.hpp:147-235).
 * SWITCHING A RECORDING BETWEEN CALLS.  This flag and every recording below (levels, breaks, bands, regions, history) may be
 * switched between two calls of hml_iterate / hml_iterate_many, also after sweeps have been recorded and also for one chain of
 * a batch alone: a switch governs the sweeps enqueued from then on.  A recording that is off skips its sweeps - the recorded
 * sweeps; for the history, the sweeps whose number is a multiple of `every` - and keeps what it has accumulated and its own N;
 * switched on again - with the same edges, regions or `every` - it goes on adding to the same accumulators.  Every recording
 * counts its own N, the sweeps recorded while IT was on; hml_recorded_sweeps is the marginals' N and grows only while the
 * marginals flag is on, whatever the other recordings do.  A read-out in the middle of a run settles the chain, reads, and
 * changes nothing: the run continues as if it had not been taken. */
typedef void (*hml_record_cb)(hml_ctx* ctx, uint64_t sweep_in_call, void* user);
int hml_set_recording(hml_ctx* ctx, int marginals, hml_record_cb cb, void* user);

/* Options.  "weight_keys" (before the observations are loaded), 1 (default): the per-sweep block scan reads a
 * one-byte-per-16-positions summary of the breakpoint weights (largest monotone 8-bit key of the group) and opens only
 * the groups that can hold a block start, comparing their float weights exactly (sweeps whose compression is
 * below 24 positions per block stream the floats instead); 2: the summary at any compression; 0: always stream all T
 * float weights.  Same block structures every way (exact). */
int hml_set_option(hml_ctx* ctx, const char* name, int value);
/* "max_blocks" (before the observations are loaded; univariate models): the BLOCK CAPACITY of the context's per-block buffers
 * (block starts, statistics, emission terms, trellis rows, maps, states) - by default T, the worst case of every position a
 * block (about 100 bytes per position: 10 GB at 10^8 positions and 5 states), and max(2^20, T / 16) for a context attached
 * to another one's observations (hml_attach_observations).  A sweep whose enumeration finds more blocks writes nothing beyond
 * the capacity and halts the chain on the device; the host then allocates larger buffers and runs the missing sweeps again,
 * with the same results (hml_stats.buffer_growths counts how often).  0: the default.  Environment: HML_MAX_BLOCKS. */
/* "fused_blocks" (any time), 1 (default): dynamic sweeps take the fused block kernel (block scan + block statistics +
 * emission terms in one launch; its workgroups hand block offsets to each other inside the launch, with a bounded
 * wait: when the GPU is shared and a wait expires the waiting workgroup computes the missing word itself, and the chain
 * takes the other path from the next sweep on); 0: always the scan + scatter + statistics launches, which share
 * nothing inside a launch - the setting for a GPU that several processes use; 2: like 1, but keep the kernel after an
 * expired wait (tests).  Same results every way.  Environment: HML_FUSED_BLOCKS.
 * "trellis_L" (any time): chunk length of the fused trellis kernels that weakly compressed univariate FB sweeps take
 * (millions of blocks; hml_k_trellis.h).  0 (default): chosen from the number of blocks and then, after 48 such sweeps,
 * by measurement - every candidate length runs two sweeps between a pair of events and the fastest stays; a multiple of
 * 32 up to 1024: that length.  A launch geometry only: rows, maps and draws are addressed by block, so the chain's
 * results are the same for every length.  Environment: HML_TRELLIS_L, HML_TRELLIS_TUNE=0 (no measurement).
 * "compat" (before hml_set_model), 0 (default) / 1: the REFERENCE-COMPATIBLE mode.  The default path addresses every
 * random decision by a Philox counter, uses its own logf / powf, sums block statistics over a fixed tree and counts in
 * exact integers: same posterior, but a chain of its own for every seed.  With compat = 1 a
 * sweep is computed exactly as the reference's single thread computes it - one std::mt19937 seeded like
 * `rng_t RNG(seed)` (src/main.cpp:107-108) and consumed in its order, glibc's expf / logf / powf bit for bit
 * (hml_math_glibc.h), float Kahan sums in block order, `size_t += float` counts - so that a run with the reference's
 * seed leaves the reference's states, parameters and marginals.  The order-dependent part of a sweep keeps the reference's
 * order but runs in chunks that are checked against each other (hml_k_compat.h; a few milliseconds per sweep of config 3's
 * 1.8 10^5 blocks - the default path is the fast one: 0.056 ms).  2 .. 64 states, like the default path (which takes the
 * number of states as a run-time value from 17 states on: hml_k_wide.h).  Environment: HML_COMPAT. */

/* hml_iterate for SEVERAL chains at once: `iterations` sweeps of every chain, sweep i of all chains before sweep i + 1.
 * Chains that live on one device, have the same shape (positions, states) and are in the strongly compressed regime of a
 * univariate Forward-Backward sweep are BATCHED: every kernel of the sweep is launched once for all of them (the chain
 * is the grid's second dimension), so the host pays for one chain's launches - a single such chain is bound by latency
 * and leaves most of the GPU idle.  Chains that share ONE construction (hml_attach_observations) additionally take one
 * block kernel for up to eight of them (block starts, statistics and emission terms of all chains from one pass over the
 * shared summary / weights / integral array): eight chains of 10^8 positions and 5 states reach 2.5 times one chain's rate.  Everything else (other shapes or devices, mixture sweeps, weakly compressed,
 * multivariate or reference-compatible chains) is run chain by chain inside the same call.  A chain's results are the
 * same bit for bit as under hml_iterate; recorded sweeps call each chain's callback in chain order. */
int hml_iterate_many(hml_ctx* const* ctxs, int n, char method, uint64_t iterations, uint64_t thinning);

/* wait for all enqueued work; surfaces model errors raised on the device */
int hml_sync(hml_ctx* ctx);

/* ---- probes: state of the last sweep (y.start()/end()/blockSize()/suffStat(), q.states(),
 * theta/A/pi values; src/Emissions.hpp:66-99, src/StateSequence.hpp:71-74) ---- */
int hml_get_num_blocks(hml_ctx* ctx, uint64_t* B);
int hml_get_blocks(hml_ctx* ctx, uint32_t* starts /* B+1, last = T */);
int hml_get_block_stats(hml_ctx* ctx, float* sum /*D*B, dimension-major*/, float* sum_sq /*D*B*/);
int hml_get_states(hml_ctx* ctx, int16_t* q /*B*/);
int hml_get_theta(hml_ctx* ctx, float* mean_var /*2K: mean0,var0,mean1,...*/);
int hml_get_transitions(hml_ctx* ctx, float* A /*K*K row-major*/, float* pi /*K*/);
int hml_set_parameters(hml_ctx* ctx, const float* mean_var, const float* A, const float* pi);
int hml_get_threshold(hml_ctx* ctx, float* thr);
/* E_s of src/StateSequence/ForwardBackward.hpp:74-81 for every block of the last sweep and the
 * normalised forward rows alpha_t (row 0 = pi); only filled when probes are enabled. */
int hml_enable_probes(hml_ctx* ctx, int on);
int hml_get_block_loglik(hml_ctx* ctx, float* E /*B*K*/);
int hml_get_forward_rows(hml_ctx* ctx, float* rows /*(B+1)*K*/);
/* sufficient statistics of the last sweep's count pass (ForwardBackward.hpp:170-200) */
int hml_get_counts(hml_ctx* ctx, uint64_t* trans /*K*K*/, uint64_t* occ /*K*/, float* sum /*K*/,
                   float* sum_sq /*K*/, uint64_t* nterms /*K*/);
/* construction probes */
int hml_get_weights(hml_ctx* ctx, float* w /*T*/);
int hml_get_coefficients(hml_ctx* ctx, float* c /*T*/);   /* maxlet coefficients (before weights) */
int hml_get_integral_array(hml_ctx* ctx, float* sum /*T+1*/, float* sum_sq /*T+1*/);

/* ---- results ---- */
/* StateMarginals (src/StateMarginals.hpp:51-137,268-310): run-length form.  Call with
 * seg_len == NULL to obtain the number of segments and of printed state columns. */
int hml_marginals_rle(hml_ctx* ctx, uint64_t* n_segments, int* n_columns, uint64_t* seg_len /*n_segments*/,
                      int32_t* counts /*n_segments * n_columns*/);
/* Maximum-posterior-margin segmentation of the recorded marginals, computed on the device - the post-processing
 * step of src/tools/maxSegmentation.cpp:53-82 without the round trip through the marginals file: arg-max state of
 * every marginal segment (first maximum; state 0 if all counts are zero), adjacent segments of equal state merged.
 * Call with run_len == NULL to obtain the number of runs. */
int hml_max_segmentation(hml_ctx* ctx, uint64_t* n_runs, uint64_t* run_len /*n_runs*/, int32_t* run_state /*n_runs*/);
/* dense per-position counts, [K+1][T] int32 on the DEVICE (row K = 1 at segment boundaries), with
 * the state rows permuted by `perm` (perm[new] = old; NULL = identity): the buffer that the
 * chain-parallel pooling all-reduces over RCCL. */
int hml_marginals_dense_device(hml_ctx* ctx, void* out_dev, const int32_t* perm);
int hml_recorded_sweeps(hml_ctx* ctx, uint64_t* n);

/* ---- emission levels per position: the denoised trace.  No counterpart in the reference. ----
 * The LEVEL of a recorded sweep at position t and data dimension d is the mean of the emission parameter of the state
 * that covers t - parameter (s / P^d) % P of state s, the mapping of hml_set_dimensions - under the theta that is current
 * AFTER that sweep's parameter update: what hml_get_theta returns inside the sweep's record callback and what the
 * parameters file prints for the sweep.  The context accumulates, per position, the sum of the levels and the sum of their
 * squares over the recorded sweeps, in double; posterior mean S1 / N and standard deviation sqrt(max(0, S2 / N - (S1 / N)^2)).
 * Memory: 2 D (T + 1) doubles and (T + 32) / 32 words, allocated by the first recorded sweep that needs them; cost per
 * recorded sweep: proportional to the number of changes of state, like the marginals.
 * hml_set_level_recording: at any time, for the sweeps recorded from then on (switching between calls: hml_set_recording);
 * turning it off keeps what was accumulated.  Off by
 * default (a sweep then launches what it launched before ABI 4).  Environment: HML_LEVELS=1. */
int hml_set_level_recording(hml_ctx* ctx, int on);
/* Run-length form: segments are cut wherever any recorded sweep had a boundary between runs of equal states.  sum[d *
 * n_segments + i] = S1 and sum_sq[...] = S2 of dimension d on segment i; n_recorded = N.  Call with seg_len == NULL to
 * obtain n_segments and n_recorded.  The sums are the same bits on every run of the same chain (fixed summation tree).
 * HML_ERR_ARG on a context that never recorded levels. */
int hml_levels_rle(hml_ctx* ctx, uint64_t* n_segments, uint64_t* n_recorded, uint64_t* seg_len /*n_segments*/,
                   double* sum /*D*n_segments, dimension-major*/, double* sum_sq /*D*n_segments*/);
/* Dense form on the DEVICE: float [2 D][T], row 2 d the posterior mean of dimension d, row 2 d + 1 its standard deviation
 * (both computed in double, then rounded once; not-a-number when nothing was recorded). */
int hml_levels_dense_device(hml_ctx* ctx, void* out_dev /* float [2D][T] */);
/* Adds `src`'s accumulators, boundary bits and count of recorded sweeps into `dst`; `src` is unchanged and `dst` may go on
 * recording.  Same device, T and D, otherwise HML_ERR_ARG (chains on different GPUs: hml_recording_merge_across, below).  Unlike the pooled
 * marginals (hml_pool_*, below) this needs NO common labels: the marginals count states, and two chains - or two halves of
 * one - may call the same level "state 1" and "state 3", so pooling them relies on hml_relabel_permutation's ordering by
 * the last sampled means; the level itself is the same number whatever the state is called, so sums over sweeps and
 * chains are exact statements about the posterior, also with twin or unused states. */
int hml_levels_merge(hml_ctx* dst, hml_ctx* src);
/* Sums of the recorded levels over caller-given segments (ABI 5): the n_cuts ascending cuts in (0, T) divide the positions
 * into n_cuts + 1 segments; sum[d * (n_cuts + 1) + k] = the sum over the positions t of segment k of S1[t], sum_sq[...] of
 * S2[t].  The cuts need not be boundaries of the levels: a fine segment that a cut splits contributes by length.  A
 * segment's mean level is sum / (N len) and its pooled spread sqrt(max(0, sum_sq / (N len) - mean^2)) with N of
 * hml_levels_rle.  Same bits on every run (the fixed summation tree of hml_levels_rle over length x value).  HML_ERR_ARG on
 * unsorted or out-of-range cuts and on a context that never recorded levels. */
int hml_levels_on_segments(hml_ctx* ctx, uint64_t n_cuts, const uint32_t* cuts /*n_cuts, ascending, in (0, T)*/,
                           double* sum /*D*(n_cuts+1), dimension-major*/, double* sum_sq /*D*(n_cuts+1)*/);

/* ---- agreement of chains on the emission level: R-hat per position (an addition to ABI 5).  No counterpart in the reference. ----
 * Do the chains that hml_levels_merge is about to add up tell the same story?  A chain's S1 and S2 at a position are the
 * sufficient statistics of the Gelman-Rubin potential scale reduction of the level there, and like the level the diagnostic
 * does not depend on what a state is called: twin states and switched labels neither fake disagreement nor hide it.
 * INPUT: n contexts, 2 <= n <= 64, distinct, on one device, with the same T and D, each with recorded levels and the same
 * N >= 2.  The contexts are only read: accumulators, bitmaps, counters and later recording are untouched.  Every context is
 * settled, the device is bound, the work runs on ctxs[0]'s stream.
 * SEGMENTS: the union of the chains' level boundaries, U of them.  On a union segment every chain's (S1, S2) is constant: the
 * values of the chain's own hml_levels_rle segment that contains it, the same bits.
 * ARITHMETIC per union segment and dimension, all in double, in this order, without contraction; the sums over the chains run
 * from chain 0 upward, starting at 0.0:
 *     m_c  = S1_c / N
 *     q_c  = S2_c / N - m_c * m_c ;  if !(q_c > 0) q_c = 0           (a chain's population variance)
 *     w0   = (sum_c q_c) / n
 *     mbar = (sum_c m_c) / n
 *     between = (sum_c (m_c - mbar) * (m_c - mbar)) / (n - 1)        (the variance of the chain means, B / N)
 *     within  = w0 * (N / (N - 1))                                    (W)
 *     rhat    = sqrt((w0 + between) / within)   if within > 0
 *             = 1                               if within == 0 and between == 0
 *             = +infinity                       if within == 0 and between > 0
 * MEANING: identical chains give between == 0 and rhat = sqrt((N - 1) / N) < 1; values near 1: the chains tell the same story
 * at that position; values well above 1: they sit in different modes there.
 * CANCELLATION: q_c is a difference of nearly equal numbers when a chain's level hardly moved; its absolute error is bounded
 * by E2 / N + 2 |m| E1 / N with the bounds E1, E2 of the segment sums (2^-52 M N (N + 1) max|mu| and the same with max mu^2: at
 * most N rounded additions into a cell, M in the scan).  A chain whose level never moved can therefore show a tiny positive
 * q_c, and a segment on which no chain's level moved a finite rhat instead of 1 or +infinity.
 * HML_ERR_ARG, each with a message of its own: a null argument, n outside 2 .. 64, a context given twice, chains on different
 * GPUs (merge their levels payloads into contexts of one device first: hml_recording_merge_payload), different T or D, a context
 * that never recorded levels, N < 2, unequal N.
 * hml_levels_agreement_rle: within, between and rhat per union segment, [d * n_segments + i]; each of the three may be NULL.
 * Call with seg_len == NULL for n_segments and n_recorded. */
int hml_levels_agreement_rle(hml_ctx* const* ctxs, int n, uint64_t* n_segments, uint64_t* n_recorded, uint64_t* seg_len /*n_segments*/,
                             double* within /*D*n_segments, dimension-major*/, double* between /*D*n_segments*/, double* rhat /*D*n_segments*/);
/* Dense form on the DEVICE: float [D][T], rhat computed in double and rounded once. */
int hml_levels_agreement_dense_device(hml_ctx* const* ctxs, int n, void* out_dev /* float [D][T] */);
/* Per dimension: the positions with rhat > threshold (+infinity included), the largest finite rhat (0 if there is none) and
 * the positions with rhat == +infinity.  Positions are counted in 64-bit integers over the union segments' lengths: exact. */
int hml_levels_agreement_summary(hml_ctx* const* ctxs, int n, double threshold, uint64_t* n_above /*D*/, double* max_finite /*D*/,
                                 uint64_t* n_infinite /*D*/);

/* ---- breakpoint posteriors per position and the consensus segmentation (ABI 5).  No counterpart in the reference. ----
 * A recorded sweep has a BREAKPOINT at position t (0 < t < T) iff a block starts at t whose state differs from the state of
 * the block before it; position 0 is never one.  The context counts, per position, the recorded sweeps with a breakpoint
 * there (C[t]) and the sweeps recorded while the recording was on (N).  Like the emission level the indicator does not
 * depend on what the states are called, so it adds over sweeps and chains without relabelling; all of it is integers, so
 * every result below is exact.  Memory: T + 1 words and (T + 32) / 32 words, allocated by the first recorded sweep that
 * needs them; cost per recorded sweep: one launch, proportional to the number of blocks.
 * hml_set_break_recording: at any time, for the sweeps recorded from then on (switching between calls: hml_set_recording);
 * turning it off keeps what was accumulated.  Off by
 * default (a sweep then launches what it launched before ABI 5).  Environment: HML_BREAKS=1. */
int hml_set_break_recording(hml_ctx* ctx, int on);
/* The positions with C > 0, ascending, and their counts; n_recorded = N.  Call with pos == NULL to obtain n_breaks and
 * n_recorded.  A context that recorded but saw no breakpoint returns n_breaks = 0; HML_ERR_ARG on a context that never
 * recorded breaks. */
int hml_breaks_list(hml_ctx* ctx, uint64_t* n_breaks, uint64_t* n_recorded, uint32_t* pos /*n_breaks*/, uint32_t* count /*n_breaks*/);
/* Dense form on the DEVICE: out[t] = (sum of C[u] over |u - t| <= window) / N - the posterior probability of a breakpoint
 * at t for window 0, the expected number of breakpoints near t otherwise.  The sum is exact (64-bit integers), the quotient
 * is taken in double and rounded once to float; not-a-number when N = 0. */
int hml_breaks_dense_device(hml_ctx* ctx, void* out_dev /* float [T] */, uint32_t window);
/* Adds `src`'s counts, positions and N into `dst`; `src` is unchanged and `dst` may go on recording.  Same device and T,
 * otherwise HML_ERR_ARG (chains on different GPUs: hml_recording_merge_across, below).  No common labels are needed. */
int hml_breaks_merge(hml_ctx* dst, hml_ctx* src);
/* Consensus breakpoints.  The candidates are the listed positions t_i with counts C_i; mass_i = the sum of C_j over
 * |t_j - t_i| <= window.  Candidate i is SELECTED iff mass_i >= max(min_count, 1) and no other candidate j within the
 * window has C_j > C_i, or C_j == C_i with t_j < t_i - whether j is selected itself plays no part, so every candidate is
 * decided on its own.  Output, ascending: position, mass and peak = C_i.  Call with pos == NULL to obtain n_selected. */
int hml_breaks_consensus(hml_ctx* ctx, uint32_t window, uint64_t min_count, uint64_t* n_selected, uint32_t* pos /*n_selected*/,
                         uint64_t* mass /*n_selected*/, uint32_t* peak /*n_selected*/);

/* ---- label-free marginals: the posterior of the emission level in caller-given bands.  No counterpart in the reference. ----
 * EDGES: n_edges floats, 1 <= n_edges <= 31, finite and strictly ascending; they define n_edges + 1 BANDS.  band(mu) = the
 * number of j with edges[j] <= mu, compared in float: band 0 lies below edges[0], band b is [edges[b-1], edges[b]), a level
 * equal to an edge belongs to the band above it, a level that is not a number to band 0.  The LEVEL of a recorded sweep at
 * position t and dimension d is the one of the emission levels above: mu of parameter (s / P^d) % P of the state s that
 * covers t, under the theta that is current after that sweep's parameter update.  COLUMNS: n_columns = D (n_edges + 1),
 * column d (n_edges + 1) + b; more than 64 columns are refused.  The context counts, per position and column, the recorded
 * sweeps whose level fell into the band, and N, the sweeps recorded while the recording was on.  The counts do not depend on
 * what a state is called - twin states, label switching and pooled chains need no relabelling - and they are integers, so
 * every result below is exact.  Segments: a boundary lies where the band of any dimension changes in any recorded sweep;
 * adjacent runs of different states in the same bands leave none, so the band segments are coarser than the levels' and the
 * marginals'.  Memory: 4 n_columns (T + 1) bytes and (T + 32) / 32 words, allocated by the first recorded sweep that needs
 * them; cost per recorded sweep: one launch, proportional to the number of blocks.
 * hml_set_level_bands sets the edges and turns the recording on, at any time, for the sweeps recorded from then on; n_edges = 0 turns it
 * off and keeps what was accumulated, and its edges.  Once a sweep has been recorded, edges that differ in any bit are
 * HML_ERR_ARG.  Off by default (a sweep then launches what it launched before).  Environment: HML_BANDS="e0,e1,...".
 * hml_get_level_bands: the edges last set (edges may be NULL). */
int hml_set_level_bands(hml_ctx* ctx, int n_edges, const float* edges /*n_edges*/);
int hml_get_level_bands(hml_ctx* ctx, int* n_edges, float* edges /*31*/);
/* Run-length form, in the shape of hml_marginals_rle: counts[i * n_columns + col] of segment i; n_recorded = N.  Call with
 * seg_len == NULL to obtain the sizes.  Per segment the columns of a dimension sum to N.  A context that was asked but recorded
 * nothing answers one segment of zeros with N = 0; HML_ERR_ARG on a context that never recorded bands. */
int hml_bands_rle(hml_ctx* ctx, uint64_t* n_segments, int* n_columns, uint64_t* n_recorded, uint64_t* seg_len /*n_segments*/,
                  int32_t* counts /*n_segments * n_columns, segment-major*/);
/* Dense form on the DEVICE: int32 [n_columns][T].  cumulative = 0: the count per band.  cumulative = 1: row b of dimension d
 * holds the sweeps whose level lay in band b or above - the exceedance count of edge b - 1; row 0 is N everywhere. */
int hml_bands_dense_device(hml_ctx* ctx, void* out_dev /* int32 [n_columns][T] */, int cumulative);
/* A call per band segment and dimension; adjacent segments whose call agrees in every dimension form one run.  rank = 0: the
 * band with the largest count (the first maximum wins, hml_max_segmentation's rule).  1 <= rank <= N: the band of the
 * rank-th smallest recorded level, i.e. the smallest b whose cumulative count over bands 0 .. b reaches rank (rank =
 * ceil(N / 2): the median's band).  Any other rank is HML_ERR_ARG.  run_band[d * n_runs + r].  Call with run_len == NULL to
 * obtain n_runs. */
int hml_bands_call(hml_ctx* ctx, uint64_t rank, uint64_t* n_runs, uint64_t* run_len /*n_runs*/, int32_t* run_band /*D*n_runs, dimension-major*/);
/* Adds `src`'s cells, boundary bits and N into `dst`; `src` is unchanged and `dst` may go on recording.  Same device, T, D and
 * bit-identical edges, otherwise HML_ERR_ARG (chains on different GPUs: hml_recording_merge_across, below); a `dst` that was never
 * given edges takes `src`'s. */
int hml_bands_merge(hml_ctx* dst, hml_ctx* src);

/* ---- joint posteriors over caller-given regions.  No counterpart in the reference. ----
 * A region is a half-open range of positions [start, end), 0 <= start < end <= T: a gene, an exon, a consensus segment.  The
 * recordings above are per position, and the positions of a region are strongly correlated within a sweep: whether the WHOLE
 * region is one segment, whether ALL of it lies in one band, how far its mean level spreads - none of these follows from
 * them.  So every recorded sweep (its blocks, its states, and theta after its parameter update: the pairing of the levels)
 * gives, per region, with blk(p) the block that holds position p, ba = blk(start), be = blk(end - 1):
 *   nb     the breakpoints strictly inside: the blocks b in (ba, be] whose state differs from that of block b - 1;
 *   same_d per data dimension d, with edges only: every block of [ba, be] has its level of dimension d in one band j_d - the
 *          bands of hml_set_level_bands (band = the number of edges <= the level, as floats; not a number: band 0), over the
 *          REGIONS' OWN edges, which have nothing to do with the edges of the per-position bands;
 *   m_d    the region's mean level, (1 / (end - start)) sum over b of (positions of block b inside the region) x level, in double.
 * and accumulates, per region,
 *   whole += (nb == 0), breaks_sum += nb, breaks_sq += nb^2 (saturating at 2^64 - 1, and staying there),
 *   level_sum[d] += m_d, level_sq[d] += m_d^2, inband[d (n_edges + 1) + j_d] += 1 when same_d.
 * N counts the sweeps recorded while the regions were on.  Everything is label-free: the sums add over sweeps, chains and GPUs.
 * The integers are exact; the double sums are the same bits on every run and depend on the sweep's blocks, states, theta and
 * the region alone (not on launch geometry, block capacity, sweep path or hml_iterate_many); their error bound is in
 * DESIGN.md 3c''''''.  A level that is not a number counts as band 0 and makes double sums not a number: those of
 * every region that holds a block of that level, and - the blocks between a region's ends are summed through running sums over
 * the sweep's blocks - those of every region that reaches beyond the chunk of 256 blocks with such a block.
 *
 * hml_set_regions gives up to 2^22 regions - in any order, overlapping, nested or repeated, each with accumulators of its own -
 * and 0 to 31 edges (the rules of hml_set_level_bands; D (n_edges + 1) <= 64), and turns the recording on.  n = 0 turns it off
 * and keeps the regions and what was accumulated; the same regions and edges, bit for bit, turn it on again.  Other regions or
 * edges replace the buffers while N = 0 and are refused afterwards.  Regions given before the observations are loaded are
 * compared with T by the first recorded sweep, which fails with a message.  hml_get_regions: what was last set (any pointer
 * but n may be NULL). */
int hml_set_regions(hml_ctx* ctx, uint64_t n, const uint32_t* start /*n*/, const uint32_t* end /*n*/, int n_edges, const float* edges /*n_edges*/);
int hml_get_regions(hml_ctx* ctx, uint64_t* n, uint32_t* start /*n*/, uint32_t* end /*n*/, int* n_edges, float* edges /*31*/);
/* The raw sums (after hml_settle).  n_columns = D (n_edges + 1), 0 without edges.  NULL arrays: the sizes only.  A context
 * that was given regions but recorded nothing answers zeros with N = 0; HML_ERR_ARG on one that was never given regions. */
int hml_regions_read(hml_ctx* ctx, uint64_t* n, int* n_columns, uint64_t* n_recorded, uint64_t* whole /*n*/, uint64_t* breaks_sum /*n*/,
                     uint64_t* breaks_sq /*n*/, double* level_sum /*D*n, dimension-major*/, double* level_sq /*D*n*/,
                     uint64_t* inband /*n*n_columns, region-major*/);
/* Adds raw sums of the same regions from anywhere - another process included - and n_recorded to N: the integers add
 * (breaks_sq with its saturation), every double gets ONE addition, ctx's value + the given one. */
int hml_regions_add(hml_ctx* ctx, uint64_t n_recorded, const uint64_t* whole, const uint64_t* breaks_sum, const uint64_t* breaks_sq,
                    const double* level_sum, const double* level_sq, const uint64_t* inband /*NULL without edges*/);
/* hml_regions_read of `src` into hml_regions_add of `dst`: same T, D, regions and edges, bit for bit, otherwise HML_ERR_ARG; the
 * two contexts may lie on any two devices.  `src` is unchanged and `dst` may go on recording. */
int hml_regions_merge(hml_ctx* dst, hml_ctx* src);

/* ---- the chain's history: a row of scalars per sweep, and convergence diagnostics over chains.  No counterpart in the
 * reference. ----
 * Every read-out above assumes that the chains behind it have converged to the same mode; the history is what shows whether
 * they have: a scalar to plot against the sweep number, a burn-in to read off, R-hat and an effective sample size over chains.
 * A row is the state of the chain AFTER a sweep - the sweep's states q through the counts hml_get_counts returns (transition
 * counts N(i,j), occupancies n(s), float sums Sx(p), Sxx(p): the numbers the conjugate update used) under the theta, A and pi
 * that the sweep's update drew - as HML_HISTORY_COLS doubles:
 *    0 sweep         the chain's sweep counter after this sweep
 *    1 method        0: forward-backward sweep, 1: mixture sweep
 *    2 ll_emit       -sum_p [ n_p/2 log(2 pi var_p) + (Sxx_p - 2 mu_p Sx_p + n_p mu_p^2) / (2 var_p) ],  n_p the (position,
 *                    dimension) terms of parameter p: n(p) for D = 1, sum_s n(s) #{d: map[s][d] = p} for "-s C P D"
 *    3 ll_path       FB: log pi[first state] + sum_ij N(i,j) log A(i,j);  mixture: sum_s n(s) log pi(s)
 *    4 lprior_theta  sum_p [ -(alpha + 1) log var_p - beta / var_p - 1/2 log var_p - nu (mu_p - mu0)^2 / (2 var_p) ]
 *    5 lprior_path   sum_ij (a_ij - 1) log A(i,j) + (pi_alpha - 1) sum_s log pi(s)       (constants dropped in 4 and 5)
 *    6 segments      1 + sum_{i != j} N(i,j)
 *    7 blocks        blocks of the sweep
 *    8 states_used   #{s: n(s) > 0}
 *    9 threshold     the wavelet threshold after the update
 *   10 chain         the context's chain_id
 * N is what the sweep's count pass left, mixture sweeps included; like the reference it starts from state 0, so N holds one
 * transition from state 0 into the first block (and `segments` is one more than the runs of equal state when the first block is
 * not in state 0).  The threshold is the one of the theta just drawn - what the next sweep's enumeration uses.
 * 2 + 3 is the COMPLETE-DATA log-likelihood of the compressed model (states given), not the marginal likelihood of the
 * filter.  All arithmetic is in double on exactly widened floats, sums in a fixed order: the same chain gives the same bits
 * on every run and behind every sweep path, hml_iterate_many and graph replay included.  A product whose count (or whose
 * coefficient a - 1) is 0 is 0; everything else is stored as IEEE gives it - lprior_path is +inf when a Dirichlet draw
 * underflowed to 0 under a_off < 1.
 *
 * hml_set_history turns the history on or off for the sweeps enqueued from now on; sweep s leaves a row when s is a multiple of
 * `every` (>= 1).  Turning it off and on keeps the rows.  A sweep then launches one more small kernel behind its parameter
 * update; with the history off a sweep launches exactly what it launches without this section.  The rows stay on the device -
 * the buffer grows on the host before a call enqueues anything - until they are read; n_dropped counts rows that found no
 * room (0 unless something is wrong).  hml_history_read copies rows [first, first + n). */
#define HML_HISTORY_COLS 11
#define HML_HISTORY_LOGLIK 100    /* columns 2 + 3 */
#define HML_HISTORY_LOGPOST 101   /* columns 2 + 3 + 4 + 5 */
int hml_set_history(hml_ctx* ctx, int on, uint64_t every);
int hml_history_size(hml_ctx* ctx, uint64_t* n_rows, uint64_t* n_dropped);
int hml_history_read(hml_ctx* ctx, uint64_t first, uint64_t n, double* rows /* n * HML_HISTORY_COLS */);
int hml_history_clear(hml_ctx* ctx);
const char* hml_history_column(int col);   /* "sweep", "method", ...; NULL beyond */
/* Diagnostics of one scalar over chains, x[c * n + i] (host arrays).  Every chain is split in halves (n odd: the middle value
 * is dropped): m = 2 n_chains sequences of length h = n / 2; W = the mean of their sample variances (divisor h - 1),
 * B = h / (m - 1) sum_j (mean_j - mean)^2, var+ = (h - 1) / h W + B / h, R-hat = sqrt(var+ / W);
 * rho_t = 1 - (W - mean_j acov_j(t)) / var+ (acov with divisor h), P_0 = 1 + rho_1, P_k = rho_2k + rho_2k+1, summed until the
 * first P_k < 0 or 2 k + 1 > h - 1 with P_k replaced by min(P_k, P_k-1), tau = -1 + 2 sum P_k, ESS = m h / tau.
 * Values that are not finite are counted in n_nonfinite and make R-hat and ESS not-a-number; chain_mean and chain_sd are taken
 * over the finite ones.  A constant series gives not-a-number twice.  h < 4: HML_ERR_ARG.  Any output may be NULL. */
int hml_history_stats(const double* x, int n_chains, uint64_t n, double* rhat, double* ess, double* chain_mean /*n_chains*/,
                      double* chain_sd /*n_chains*/, uint64_t* n_nonfinite);
/* The same from contexts (any devices of this process): column `col`, or HML_HISTORY_LOGLIK / HML_HISTORY_LOGPOST; the rows with
 * sweep <= skip_sweeps are left out and the last n_used = min over the chains of the rows that remain are used of each. */
int hml_history_summary(hml_ctx* const* ctxs, int n, int col, uint64_t skip_sweeps, double* rhat, double* ess, double* chain_mean /*n*/,
                        double* chain_sd /*n*/, uint64_t* n_used, uint64_t* n_nonfinite);

/* ---- Viterbi decode: the jointly most probable state path under the current parameters.  No counterpart in the reference. ----
 * hml_max_segmentation takes the arg-max of every position's marginal on its own; this is the ONE path over the context's
 * current blocks (those of the last enumeration: a sweep's, or hml_create_blocks') that maximises
 *     log pi(q_0) + sum_b E_b(q_b) + sum_{b > 0} log A(q_{b-1}, q_b)
 * under the parameters as they stand (the last update's, or hml_set_parameters'), E_b(s) being the float block term of the
 * forward-backward sweep (hml_get_block_loglik) with the block statistics taken anew from the integral array.  Workflow for
 * a point estimate: hml_set_parameters (for example posterior means by sorted state), optionally hml_create_blocks at a
 * threshold of the caller's choice, then hml_viterbi.  The chain is only read: its next sweeps are the same with or without.
 *
 * The maximisation is carried out in FIXED POINT, so that the answer is one exact path on every device and under every
 * launch geometry: every term is an int64 in units of 2^-20 nat, fx(x) = llrint(clamp(x, -2^38, 2^38) 2^20) with not-a-number
 * taken as -2^38 (an exact 0 in A or pi is a very bad, finite score), init[j] = fx(logf pi_j), trans[i][j] = fx(logf A_ij),
 * emit[b][j] = fx(E_b(j)), logf and the terms' normalisers derived from mean, variance and A by the library's own logf
 * (a "compat" context decodes to the same tables).  d_0(j) = init[j] + emit[0][j], d_b(j) = max_i(d_{b-1}(i) + trans[i][j]) +
 * emit[b][j] with max_j d_b(j) subtracted after every block; ties go to the SMALLEST index - in the back-pointer of every
 * block and in the end state - so among the paths of maximal score the one returned is the smallest read from the last block
 * backwards.  score_fixed is the int64 sum of the path's terms (two's complement; it cannot wrap unless a term is clamped),
 * score the same in nats, (double)score_fixed / 2^20.  hammlet_amd/csrc/hml_viterbi_ref.h restates all of it for one host thread.
 *
 * hml_viterbi: run-length form over positions, adjacent blocks of equal state merged; call with run_len == NULL to obtain
 * the number of runs.  hml_viterbi_states: the path per block.  hml_viterbi_scores: the tables a decode uses (any may be
 * NULL).  Every call decodes anew, with device memory of its own that is released before it returns; the same input gives
 * the same words.  A context without blocks (no sweep and no hml_create_blocks yet) is refused.
 * hml_viterbi_info, of the last decode: chunks the blocks were cut into, their length L and warm-up W in blocks, the chunks
 * found stale after the first pass, the parallel repair rounds run, the chunks the single finishing lane ran again (any
 * may be NULL).  Options "viterbi_W", "viterbi_L" (blocks, up to 2^20; 0: the default of 64) and "viterbi_rounds" (0 ... 16,
 * default 8) are launch geometry: the result never depends on them ("Viterbi decode"). */
int hml_viterbi(hml_ctx* ctx, uint64_t* n_runs, uint64_t* run_len /*n_runs*/, int32_t* run_state /*n_runs*/, int64_t* score_fixed, double* score);
int hml_viterbi_states(hml_ctx* ctx, int16_t* q /*B*/);
int hml_viterbi_scores(hml_ctx* ctx, int64_t* emit /*B*K*/, int64_t* trans /*K*K*/, int64_t* init /*K*/);
int hml_viterbi_info(hml_ctx* ctx, uint64_t* chunks, uint64_t* L, uint64_t* W, uint64_t* stale_chunks, uint64_t* rounds, uint64_t* serial_chunks);

/* ---- smoothing: state posteriors per block and log p(y | theta).  No counterpart in the reference. ----
 * The sum over paths where hml_viterbi takes the maximum: with the weight of a path q over the context's current B blocks
 *     pi(q_0) prod_b exp E_b(q_b) prod_{b > 0} A(q_{b-1}, q_b)
 * (E_b(s) as above: the float hml_viterbi quantises), gamma[b][j] = p(q_b = j | y, theta) is the share of the paths through
 * state j at block b, and loglik = log p(y | theta) the logarithm of the sum of all weights - the MARGINAL likelihood of the
 * compressed model, which no sampled path enters (the history's ll columns are the complete-data values).  The chain is only
 * read: its next sweeps are the same with or without.
 *
 * The tables m_b = max_j E_b(j) and e_b(j) = expf(E_b(j) - m_b) are the sweep's floats.  Everything after them is IEEE double
 * on exactly widened floats in one fixed order, so that the same input gives the same words on every device and under every
 * launch geometry: the forward recursion normalised per block (a_b(j) = e_b(j) sum_i alpha_{b-1}(i) A_ij, c_b = sum_j a_b(j),
 * alpha_b = a_b / c_b), the backward recursion normalised likewise from beta_{B-1} = 1 / K, gamma_b = alpha_b beta_b over its
 * sum, and loglik = the fan-in-64 tree sum of l_b = m_b + log c_b.  A block no path reaches (c_b not a positive finite number)
 * is DEGENERATE: alpha_b restarts from 1 / K, loglik is what IEEE gives (-inf or not-a-number) and `degenerate` counts such
 * blocks; gamma holds no not-a-number.  hammlet_amd/csrc/hml_posterior_ref.h states every step and restates it for one host
 * thread.
 *
 * hml_posterior: gamma (may be NULL), loglik, degenerate (either may be NULL).  hml_posterior_rle: the call per position -
 * per block the smallest state at the maximum of gamma_b, adjacent blocks of equal state merged into runs over positions,
 * run_conf the minimum over a run's blocks of the posterior of its state; call with run_len == NULL to obtain the number of
 * runs (run_state and run_conf may be NULL).  hml_posterior_terms: the tables and rows a call uses (probe; any may be NULL).
 * Every call computes anew, with device memory of its own that is released before it returns.  A context without blocks is
 * refused.  A context always holds a transition matrix; a model meant as a mixture alone (no transitions) is not this
 * read-out's subject, and the driver refuses the output for a scheme of mixture sweeps only.
 * hml_posterior_info, of the last call: chunks the blocks were cut into, their length L and warm-up W in blocks, the chunks
 * found stale after the first pass of the forward and of the backward recursion, the parallel repair rounds run (the larger
 * of the two directions'), the chunks the single finishing lane ran again (both directions; any may be NULL).  Options
 * "posterior_W", "posterior_L" (blocks, up to 2^20; 0: the defaults of 256 and 64) and "posterior_rounds" (0 ... 16, default
 * 8) are launch geometry: no word of any result depends on them ("Smoothing"). */
int hml_posterior(hml_ctx* ctx, double* gamma /*B*K, may be NULL*/, double* loglik, uint64_t* degenerate);
int hml_posterior_rle(hml_ctx* ctx, uint64_t* n_runs, uint64_t* run_len /*n_runs*/, int32_t* run_state /*n_runs*/, double* run_conf /*n_runs*/);
int hml_posterior_terms(hml_ctx* ctx, float* e /*B*K*/, float* m /*B*/, double* alpha /*B*K*/, double* c /*B*/, double* beta /*B*K*/);
int hml_posterior_info(hml_ctx* ctx, uint64_t* chunks, uint64_t* L, uint64_t* W, uint64_t* stale_fwd, uint64_t* stale_bwd, uint64_t* rounds, uint64_t* serial_chunks);

/* ---- expectation-maximisation: expected counts, and a fit of theta, A and pi.  No counterpart in the reference. ----
 * The other half of Baum-Welch over the context's current B blocks, for the path weight stated under smoothing.  The E-step
 * runs a smoothing pass and reduces, in IEEE double and one fixed order (fan-in-64 tree sums over the blocks, as loglik's):
 *     xi[i][j]   the expected number of transitions i -> j between adjacent blocks: the sum over b = 1 ... B - 1 of
 *                alpha_{b-1}(i) A_ij e_b(j) beta_b(j) over its sum X_b (a block with X_b not a positive finite number gives
 *                zeros and is counted in xi_degenerate)
 *     first[j]   gamma_0(j)
 *     occ[j]     the expected number of positions in state j, sum_b n_b gamma_b(j); stay[j] the same with n_b - 1: the expected
 *                self-transitions inside blocks, which count for A_jj when self-transitions are on
 *     sum[j][d], sum_sq[j][d]   sum_b gamma_b(j) Sx_{d,b}, and the same with the block's sum of squares
 * and returns loglik and degenerate as hml_posterior does.  This is the E-step of that path weight, NOT the sweep's count
 * pass, which feeds pi's posterior the full occupancies and books a transition into the first block.
 * The M-step (host, K-sized) gives the theta, A and pi that maximise the expected complete-data log-likelihood - use_prior = 0,
 * maximum likelihood - or that plus the log density of the chain's own priors (hml_set_model) - use_prior = 1, the posterior
 * mode: the joint mode of the normal-inverse-gamma posterior per emission parameter, (count + a - 1) normalised per row of A
 * and for pi, negative values raised to 0.  A parameter or a row without support keeps its old values and is counted in
 * `kept`.  The result is installed exactly as hml_set_parameters installs it.  hammlet_amd/csrc/hml_em_ref.h states every step,
 * restates the E-step for one host thread, and holds the M-step and the objective the library itself calls.
 *
 * hml_expected_counts: any pointer may be NULL; the chain is only read.  hml_em_step: one E-step, the M-step and the
 * installation; objective_before is the objective of the parameters the step started from (either pointer may be NULL).
 * hml_em_fit: trace[k] is the objective - loglik, with use_prior = 1 plus the log prior density up to constants - of the
 * parameters after k M-steps.  Before each M-step the fit stops when the E-step reports degenerate + xi_degenerate > 0
 * (HML_EM_DEGENERATE), when k >= 1 and trace[k] - trace[k-1] <= rel_tol |trace[k-1]| (HML_EM_CONVERGED), or after max_steps
 * M-steps (HML_EM_MAX_STEPS), so that it runs at most max_steps M-steps and one E-step more, and the last trace entry always
 * belongs to the installed parameters.  steps = the M-steps run (trace holds steps + 1 values), kept sums over them.
 * BLOCKS ARE NEVER REBUILT inside a fit: it is over the context's current block structure, as the decode and the smoothing
 * are; a caller who wants the threshold to follow the fitted parameters calls hml_create_blocks between fits.  The refusals
 * are hml_posterior's (a halted chain, no blocks, no model); hml_posterior_info reports the E-step's last smoothing pass.
 * Device memory is local to a call and released before it returns. */
#define HML_EM_MAX_STEPS 0
#define HML_EM_CONVERGED 1
#define HML_EM_DEGENERATE 2
int hml_expected_counts(hml_ctx* ctx, double* xi /*K*K*/, double* first /*K*/, double* stay /*K*/, double* occ /*K*/, double* sum /*K*D*/, double* sum_sq /*K*D*/,
                        double* loglik, uint64_t* degenerate, uint64_t* xi_degenerate);
int hml_em_step(hml_ctx* ctx, int use_prior, double* objective_before, uint64_t* kept);
int hml_em_fit(hml_ctx* ctx, int use_prior, uint64_t max_steps, double rel_tol, double* trace /*max_steps+1, may be NULL*/, uint64_t* steps, int* reason, uint64_t* kept);

/* ---- EM from many starts: a batch of fits smoothed together, the best kept.  No counterpart in the reference. ----
 * hml_em_fit is deterministic and climbs to the local optimum its start leads to.  hml_em_fit_many runs R fits over the same
 * blocks from R starts.  MEMBER r IS EXACTLY hml_set_parameters(start_r) FOLLOWED BY hml_em_fit(use_prior, max_steps, rel_tol)
 * ON THIS CONTEXT: its trace, steps, reason, kept and fitted floats are those, word for word, whatever R is, whoever else is in
 * the batch and however the batch is cut.  On the device the members still running share one set of launches per E-step (the
 * member is a grid dimension); the stopping rule, the objective and the M-step run per member on the host, as in hml_em_fit.
 *   R             1 ... 4096 members; start r is mean_var[r], A[r], pi[r].  Every start is checked as hml_set_parameters checks
 *                 it before anything is launched; a bad one is refused with that function's message and the member's index,
 *                 and nothing is changed.  The other refusals are hml_posterior's.
 *   outputs       any may be NULL.  trace[r] holds max_steps + 1 entries, those past the member's last are NaN; objective[r] is
 *                 the member's last trace entry.
 *   best          the candidates are the members whose reason is not HML_EM_DEGENERATE and whose objective is finite; best is
 *                 the candidate with the greatest objective, the smallest index among equals, and -1 without a candidate (the
 *                 call still returns 0).  hammlet_amd/csrc/hml_em_many_ref.h holds the rule the library calls.
 *   install       The context's parameters are not touched while the batch runs.  install != 0 and best >= 0: the winner's
 *                 floats are installed through hml_set_parameters at the end, which leaves the context as a single hml_em_fit
 *                 from that start would have.  Otherwise the chain is only read.
 * Device memory is local to the call and bounded: the members run in groups of as many as fit hml_set_em_batch_bytes' budget
 * (0: the default, 4 GiB; a member needs about 2 B K 8 bytes for alpha and beta and little else; at least one member a group).
 * hml_em_starts fills R starts: member 0 is the context's current parameters; for r >= 1 the means are drawn uniformly over
 * the current means' range widened by `spread` (finite, positive; 1 is a fair default) and sorted ascending, the variances
 * between a quarter and twice the current mean variance, from Philox words addressed by (seed, r, parameter) - the header above
 * states every operation; A and pi (either may be NULL) are the current ones for every member.
 * hml_em_many_info, of the last hml_em_fit_many: members = R; groups and group_size of the first E-step; esteps = E-steps of
 * the longest member; launch_sets = first-pass launches of the forward direction, one per group and E-step (groups x esteps
 * while every member runs); stale_fwd, stale_bwd and serial_chunks summed over members and E-steps, rounds the maximum. */
int hml_em_fit_many(hml_ctx* ctx, uint64_t R, const float* mean_var /*R*2P*/, const float* A /*R*K*K*/, const float* pi /*R*K*/, int use_prior, uint64_t max_steps,
                    double rel_tol, int install, double* trace /*R*(max_steps+1)*/, uint64_t* steps /*R*/, int* reason /*R*/, uint64_t* kept /*R*/,
                    float* fit_mean_var /*R*2P*/, float* fit_A /*R*K*K*/, float* fit_pi /*R*K*/, double* objective /*R*/, int64_t* best);
int hml_em_starts(hml_ctx* ctx, uint64_t R, uint64_t seed, double spread, float* mean_var /*R*2P*/, float* A /*R*K*K*/, float* pi /*R*K*/);
int hml_em_many_info(hml_ctx* ctx, uint64_t* members, uint64_t* groups, uint64_t* group_size, uint64_t* esteps, uint64_t* launch_sets, uint64_t* stale_fwd,
                     uint64_t* stale_bwd, uint64_t* rounds, uint64_t* serial_chunks);
int hml_set_em_batch_bytes(hml_ctx* ctx, uint64_t bytes /*0: the default*/);

/* ---- pairwise read-outs of the smoothing: breakpoint and region posteriors under the current parameters.  No counterpart in
 * the reference. ----
 * The joint questions of "joint posteriors over regions" above, asked of a fitted model instead of recorded sweeps: where the
 * breakpoints are and how sure each is, whether a whole region is one segment or all of it in one state, how many breakpoints
 * to expect inside it.  Under fixed parameters these are exact functions of the rows alpha and beta of a smoothing pass - no
 * Monte-Carlo error - and none of them follows from gamma.  They bear labels, which a fitted model can afford.
 * With e, alpha, beta, gamma as smoothing defines them, IEEE double, + x / only, sums from 0.0 in ascending index:
 *   per boundary b = 1 ... B - 1 (between blocks b - 1 and b):  v(j) = e_b(j) beta_b(j);  x(i, j) = (alpha_{b-1}(i) A_ij) v(j);
 *     d_b = sum_j x(j, j);  o_b = sum_i sum_{j != i} x(i, j) (i outer, j inner);
 *     p_b = o_b / (d_b + o_b), the posterior probability of a change of state at position starts[b].  The off-diagonal mass is
 *     summed directly and never formed as one minus the rest, so a probability of 1e-20 stays one.  If d_b + o_b is not a
 *     positive finite number, p_b = 0 and the boundary is counted in pair_degenerate.
 *     u(j) = sum_k A_jk v(k);  r_b(j) = (A_jj v(j)) / u(j) = p(q_b = j | q_{b-1} = j, y, theta), and 0 where u(j) is not a
 *     positive finite number (the quotient would be 0 / 0): no output holds a not-a-number.
 *   in fixed point (integers: their prefix sums are associative, so no result depends on how a scan is cut):
 *     pfx_b = llrint(p_b 2^32);  cost_b(j) = 1023 2^22 (the cap) if u(j) is not positive finite or r_b(j) is not > 0, else
 *     min(llrint(max(-log r_b(j), 0) 2^22), cap), in units of 2^-22 nat;  mass_b(j) = n_b llrint(gamma_b(j) 2^32) for
 *     b = 0 ... B - 1.  Block 0 has no boundary: p_0, r_0, pfx_0 and cost_0 are 0.  N, C_j and G_j are their inclusive prefix
 *     sums over b, in uint64.  e^x is taken as exactly 0 below -700: one capped boundary makes a joint probability exactly 0.
 *   per region [start, end) (positions, half open, in any order, overlapping or repeated), ba and be the blocks of start and end - 1:
 *     whole_state[j]  = gamma_ba(j) exp(-(C_j[be] - C_j[ba]) 2^-22): the probability that every position of it is in state j
 *     whole           = sum_j whole_state[j]: the probability of no breakpoint inside it
 *     expected_breaks = (N[be] - N[ba]) 2^-32
 *     share[j]        = (M_j 2^-32) / (end - start), M_j the sum of mass(j) over blocks ba ... be less (start - starts[ba])
 *                       llrint(gamma_ba(j) 2^32) and (starts[be + 1] - end) llrint(gamma_be(j) 2^32): the expected fraction of
 *                       its positions in state j.  The region's expected level is sum_j share[j] mu_d(j), on the host.
 *   A cost is off by at most 2^-23 nat, so whole_state by at most (be - ba) 2^-23 relative (1e-3 over 10^4 blocks);
 *   expected_breaks by at most (be - ba) 2^-33; share[j] by at most 2^-33.  hammlet_amd/csrc/hml_pairs_ref.h states every step
 *   and restates it for one host thread; the device gives those very words.
 * hml_posterior_breaks: the boundaries with p_b >= min_prob by ascending position (pos == NULL: the count alone; prob may be
 * NULL; B - 1 entries always suffice); expected_breaks = N[B - 1] 2^-32, the expected number of breakpoints in the trace.  A
 * min_prob that is not a number is HML_ERR_ARG, and so are more than 2^31 - 1 blocks: the list's counts are 32-bit.
 * hml_posterior_regions: the regions are arguments - they are not hml_set_regions' and disturb no recording;
 * start >= end or end > T is HML_ERR_ARG; n = 0 succeeds; any output may be NULL; raw holds per region the break units
 * N[be] - N[ba], the K cost differences and the K masses M_j.  hml_posterior_pair_terms: the terms themselves (probe; any may be
 * NULL).  The refusals are hml_posterior's (a halted chain, no blocks, no model); hml_posterior_info reports the smoothing pass
 * behind the call.  The chain is only read.  Device memory - (2 K + 2) 8 bytes per block on top of the smoothing's - is local
 * to a call and released before it returns. */
int hml_posterior_breaks(hml_ctx* ctx, double min_prob, uint64_t* n, uint32_t* pos /*n*/, double* prob /*n*/, double* expected_breaks, uint64_t* pair_degenerate);
int hml_posterior_regions(hml_ctx* ctx, uint64_t n, const uint32_t* start /*n*/, const uint32_t* end /*n*/, double* whole /*n*/, double* whole_state /*n*K*/,
                          double* expected_breaks /*n*/, double* share /*n*K*/, uint64_t* raw /*n*(2K+1), may be NULL*/, uint64_t* pair_degenerate);
int hml_posterior_pair_terms(hml_ctx* ctx, double* p /*B*/, double* r /*B*K*/, uint64_t* pfx /*B*/, uint64_t* cost /*B*K*/, uint64_t* mass /*B*K*/);

/* ---- sampled paths: independent draws of whole state paths from p(q | y, theta) under the current parameters.  No counterpart
 * in the reference (its `sequences` file holds the dependent paths of the sweeps, each under its own parameters). ----
 * What no exact read-out answers under a fitted model is read off such draws: how far a breakpoint can move, whether two
 * regions change together.  (The distribution of the number of breakpoints in a region is exact: hml_posterior_region_counts
 * below.)  A sweep cannot serve: it redraws the parameters
 * and yields one dependent path.  With alpha as smoothing defines it (forward rows, degenerate restarts included) and A widened
 * exactly to double:
 *   uniform of draw r at block b:  o = Philox4x32-10 words of hml_stream4(hml_make_key(seed, 0), HML_KIND_PSAMPLE = 8, epoch r,
 *     index b >> 1, 0);  (hi, lo) = (o[0], o[1]) for even b, (o[2], o[3]) for odd b;  u = ((hi >> 5) 2^26 + (lo >> 6)) 2^-53.
 *     Draw r depends on (seed, r) alone - never on count, first, the grouping or the launch geometry.
 *   categorical rule over weights w(0 ... K - 1) in IEEE double: c_i the running sums from 0.0 in ascending i, S = c_{K-1},
 *     t = u S; the smallest i with t < c_i, or, if there is none, the largest i with w(i) > 0.  Weight 0 is never drawn.
 *   q_{B-1} from w = alpha_{B-1};  q_b, b = B - 2 ... 0, from w(i) = alpha_b(i) A[i][q_{b+1}].  If S is not a positive finite
 *     number the block is degenerate for this draw - counted in sample_degenerate - and w = alpha_b is used; if that sum fails the
 *     same test, q_b = 0.
 *   per draw: segments = 1 + #{b >= 1: q_b != q_{b-1}};  score_fixed in the tables of hml_viterbi_scores (units of 2^-20 nat,
 *     comparable with hml_viterbi's and never above it).
 *   over the draws of a call: change_count[b] = #draws with q_b != q_{b-1} (0 at b = 0);  state_count[b][j] = #draws with q_b = j.
 *   per region [start, end), ba and be as in hml_posterior_regions, n_r = #{b in (ba, be]: q_b != q_{b-1}} in draw r:
 *     hist[h], h = 0 ... H = max_breaks, the draws with n_r = h (the last bin: n_r >= H);  whole_state[j] the draws with n_r = 0
 *     and q_ba = j;  breaks_sum = sum_r n_r;  breaks_sq = sum_r n_r^2.
 * hammlet_amd/csrc/hml_sample_ref.h restates all of it for one host thread; the device gives those very words.
 * The call makes draws first ... first + count - 1; count is 1 ... 2^24 and first + count <= 2^48 (HML_ERR_ARG otherwise), so
 * ranges of `first` split a sample over calls or processes exactly.  paths is draw-major, a byte per block.  Any output may be
 * NULL.  A bad region is HML_ERR_ARG as in hml_posterior_regions, max_breaks = 0 too; n = 0 succeeds.  The refusals are
 * hml_posterior's (a halted chain, no blocks, no model).  The chain is only read.  Device memory is local to a call and
 * released before it returns: the alpha rows, and per draw of a group about B bytes (2 B with paths) plus 10 bytes per chunk;
 * the draws run in groups of as many as fit hml_set_sample_batch_bytes (at least one), and no output word depends on the
 * grouping.  Options "sample_W", "sample_L", "sample_rounds" (hml_set_option; ranges of the posterior_ ones) are launch geometry
 * only.  hml_posterior_sample_info: of the last call - the draws, their groups and the size of a full one, the chunks of a draw,
 * L, W, the (draw, chunk) pairs that were stale after the first run, the greatest number of repair rounds of a group, and the
 * pairs the finishing lanes ran. */
int hml_posterior_sample(hml_ctx* ctx, uint64_t first, uint64_t count, uint64_t seed, uint8_t* paths /*count*B, draw-major, may be NULL*/,
                         uint64_t* segments /*count*/, int64_t* score_fixed /*count*/, uint32_t* change_count /*B*/, uint32_t* state_count /*B*K*/,
                         uint64_t* sample_degenerate);
int hml_posterior_sample_regions(hml_ctx* ctx, uint64_t first, uint64_t count, uint64_t seed, uint64_t n, const uint32_t* start /*n*/, const uint32_t* end /*n*/,
                                 uint32_t max_breaks /*H >= 1*/, uint32_t* hist /*n*(H+1)*/, uint32_t* whole_state /*n*K*/, uint64_t* breaks_sum /*n*/,
                                 uint64_t* breaks_sq /*n*/);
int hml_posterior_sample_info(hml_ctx* ctx, uint64_t* draws, uint64_t* groups, uint64_t* group_size, uint64_t* chunks, uint64_t* L, uint64_t* W,
                              uint64_t* stale_first, uint64_t* rounds, uint64_t* serial_chunks);
int hml_set_sample_batch_bytes(hml_ctx* ctx, uint64_t bytes /*0: the default, 4 GiB*/);

/* ---- count read-outs of the smoothing: per region the exact distribution of the number of breakpoints, and the probability
 * that no part of it is in a given state.  No counterpart in the reference. ----
 * "How many breakpoints does this region hold?" as a distribution, not an expectation, and "does any part of it touch state j?" -
 * for a copy-number user "is any part of this gene deleted?".  whole_state is "all of it is in j", share an expectation, gamma per
 * block: none answers either.  Under fixed parameters the posterior over paths is a Markov chain over the blocks with the
 * transitions p(q_b = j | q_{b-1} = i, y, theta) = A_ij v_b(j) / u_b(i), v and u as the pairwise read-outs above define them, and
 * both answers are short forward recursions over the region's blocks on those transitions: exact, no draws, no Monte-Carlo
 * error - a probability of 1e-12 is resolved.  IEEE double, + x / only, sums from 0.0 in ascending index:
 *   per boundary b = 1 ... B - 1:  v_b(j) = e_b(j) beta_b(j);  u_b(i) = sum_k A_ik v_b(k);  rho_b(i) = 1 / u_b(i), and 0 where
 *     u_b(i) is not a positive finite number - for this purpose: not a finite number of at least 2^-1000, so that no later
 *     product can overflow: the pair (b, i) is counted in count_degenerate and the mass leaving state i there is lost rather
 *     than turned into a not-a-number.  A v_b(j) that is not a finite non-negative number (e_b(j) is a not-a-number) is
 *     replaced by 0 once u_b is formed - every rho_b is 0 then.  Block 0 has no boundary: v_0 = rho_0 = 0.
 *   per region [start, end), ba and be as in hml_posterior_regions, H = max_breaks:
 *     count cells   f(j, 0) = gamma_ba(j), f(j, h > 0) = 0;  for b = ba + 1 ... be, with phi(i, h) = f(i, h) rho_b(i):
 *                   f'(j, h) = (A_jj phi(j, h) + s(j, h)) v_b(j);  s(j, 0) = 0, s(j, h) = sum_{i != j} A_ij src(i, h);
 *                   src(i, h) = phi(i, h - 1) for 1 <= h < H, src(i, H) = phi(i, H - 1) + phi(i, H): the last bin absorbs
 *     hist[h]        = sum_j f(j, h) after block be: the probability of exactly h breakpoints inside the region; h = H: H or more
 *     whole_state[j] = f(j, 0): all of it in state j - the unquantised sibling of hml_posterior_regions' value
 *     avoidance cells, per struck-out state x:  g_x(i) = gamma_ba(i) for i != x, 0 at x;
 *                   g'_x(i) = (sum_{k != x} A_ki (g_x(k) rho_b(k))) v_b(i) for i != x, 0 at x
 *     avoid[x]       = sum_{i != x} g_x(i) after block be: the probability that no position of the region is in state x.  That
 *                      it touches x is 1 - avoid[x], exact to 2^-53 absolute; a small avoid[x] keeps its relative precision.
 *   Every operation is on non-negative numbers: nothing cancels, and a value is off by about its chain's operation count times
 *   2^-53 relative.  Without degenerate boundaries sum_h hist[h] = 1 up to rounding; otherwise the shortfall is the lost mass.
 *   No output holds a not-a-number.  hammlet_amd/csrc/hml_counts_ref.h states every step and restates it for one host thread;
 *   the device gives those very words.
 * The regions are arguments, as hml_posterior_regions' are: in any order, overlapping or repeated; start >= end or end > T is
 * HML_ERR_ARG naming the region; n = 0 succeeds; any output may be NULL.  max_breaks must be 1 ... 32 with
 * K (max_breaks + 1) <= 1024 - 32 up to 31 states, 15 at 64 - and is HML_ERR_ARG otherwise.  The other refusals are
 * hml_posterior's (a halted chain, no blocks, no model).  The chain is only read.  Device memory - 2 K 8 bytes per block on top of
 * the smoothing's - is local to a call and released before it returns.  Options "posterior_L", "posterior_W" and
 * "posterior_rounds" stay launch geometry only: no output word depends on them.
 * Cost: a region is a serial chain of be - ba steps, one wavefront walking it.  The call is meant for many regions of gene or
 * segment size; one region over a whole trace of 10^6 blocks is legal and slow.
 * hml_posterior_count_terms: v and rho themselves (probe; either may be NULL).  hml_posterior_counts_info: of the last
 * hml_posterior_region_counts - its regions, the sum of be - ba over them and the largest be - ba. */
int hml_posterior_region_counts(hml_ctx* ctx, uint64_t n, const uint32_t* start /*n*/, const uint32_t* end /*n*/, uint32_t max_breaks /*H*/,
                                double* hist /*n*(H+1)*/, double* whole_state /*n*K*/, double* avoid /*n*K*/, uint64_t* count_degenerate);
int hml_posterior_count_terms(hml_ctx* ctx, double* v /*B*K*/, double* rho /*B*K*/);                    /* probe */
int hml_posterior_counts_info(hml_ctx* ctx, uint64_t* regions, uint64_t* steps, uint64_t* longest);     /* of the last call */

/* ---- sparse payloads: levels, breakpoints and bands across GPUs.  No counterpart in the reference. ----
 * The three recordings above keep a cell and a boundary bit per change of state, so what another GPU needs of one is a list:
 * the M positions with a cell and the cells there.  The PAYLOAD is one contiguous buffer in device memory, little endian,
 * aligned to 8 bytes, of the same form for the three kinds:
 *     uint64 header[8]  [0] the magic number 0x00314345524C4D48 (the bytes "HMLREC1\0"), [1] the kind, [2] T,
 *                       [3] rows: 2 D for levels, 1 for breaks, D (n_edges + 1) for bands, [4] M, [5] N, the recorder's count
 *                       of recorded sweeps, [6] bytes per cell (8, 4, 4), [7] n_band_edges (0 unless bands)
 *     float  edges[32]  the bands' edges followed by zeros; all zero for levels and breaks
 *     uint32 pos[M]     strictly ascending, all < T: for levels and bands the positions whose boundary bit is set and the
 *                       position 0, for breaks the positions with a count (never 0); zero bytes up to a multiple of 8 bytes
 *     cells[rows][M]    cells[r * M + i] = the recorder's RAW cell of row r at pos[i] - the difference the recorded sweeps
 *                       accumulated there, not the run-length read-outs' sums: double for levels, uint32 for breaks, int32 for bands
 * Size: 192 + 8 ceil(M / 2) + rows M (bytes per cell).  A recorder that was asked for but has recorded no sweep exports
 * M = 0 and N = 0; one that was never asked for is HML_ERR_ARG, with the message of the kind's read-outs.
 * hml_recording_payload_size / hml_recording_export: the chain is settled, its boundary bitmap compacted, the cells gathered
 * and the payload written on the context's stream, which is synchronised.  capacity_bytes below the size: HML_ERR_ARG, nothing
 * is written (n_bytes, if given, still receives the size).
 * hml_recording_merge_payload: `payload_dev` lies on `dst`'s device.  dst[r][pos[i]] += cells[r * M + i], the boundary bits
 * are set and N is added - the additions of hml_levels_merge / hml_breaks_merge / hml_bands_merge, in their order, so `dst`
 * ends in the bits it would hold after that call with the exporting chain as `src`; `dst` may go on recording.  A bands
 * destination that was never given edges takes the payload's; edges that differ in any bit are refused.  Everything is checked
 * BEFORE anything is written - magic number, kind, T, rows against `dst`'s D (and the payload's edges), cell size, n_bytes
 * against the size formula, the edges, and on the device that the positions are strictly ascending, below T and, for breaks,
 * above 0: each failure is HML_ERR_ARG with a message of its own and leaves `dst` as it was.
 * hml_recording_merge_across: export on `src`'s device, the bytes to `dst`'s device (hipMemcpyPeer; none when they share
 * one), merge.  Same T (and D) as for the merges above, otherwise HML_ERR_ARG.
 * R-HAT ACROSS GPUS needs no call of its own: a context attached to a chain of the target device (hml_attach_observations),
 * with its model set and no recorded sweep, that a levels payload was merged into reads out exactly like the exporting chain
 * - the same bits from hml_levels_rle (a cell is never -0.0, so 0.0 + cell is the cell), the same N - and is accepted by
 * hml_levels_agreement_* beside the chains of that device. */
#define HML_RECORDING_LEVELS 0
#define HML_RECORDING_BREAKS 1
#define HML_RECORDING_BANDS 2
int hml_recording_payload_size(hml_ctx* ctx, int kind, uint64_t* n_bytes);
int hml_recording_export(hml_ctx* ctx, int kind, void* payload_dev, uint64_t capacity_bytes, uint64_t* n_bytes);
int hml_recording_merge_payload(hml_ctx* dst, int kind, const void* payload_dev, uint64_t n_bytes);
int hml_recording_merge_across(hml_ctx* dst, hml_ctx* src, int kind);

/* Trellis::sample(t) (src/Trellis.hpp:61-66): one draw of std::discrete_distribution over K weights - p_i = w_i / sum in
 * double, first i whose cumulative probability reaches u - with u from the chain's Philox key (sub-stream HOST,
 * one counter step per call).  Runs on the host (shared arithmetic of the kernels, hml_dist.h). */
int hml_categorical_draw(hml_ctx* ctx, const float* weights, int K, uint32_t* index);

/* ---- chain-parallel pooling.  Chains shard across GPUs and never communicate while sampling;
 * one ncclAllReduce(sum, int32) over xGMI pools their recorded state marginals at the end.  The reference has no
 * counterpart (one process, one thread, src/main.cpp:108). ---- */
/* Common labels: perm[new] = old with the states ordered by ascending emission mean of the current theta - for
 * "-s C P D" by the tuple of the means of their mapped parameters, in dimension order; ties keep their order.  (The
 * idea of bin/sortStates:1-6, which orders states by their last sampled mean.) */
int hml_relabel_permutation(hml_ctx* ctx, int32_t* perm /*K*/);
/* The payload one chain contributes: int32 [K+1][T+1] - rows 0..K-1 the relabelled per-state difference arrays of the
 * recorded marginals, row K = 1 at recorded segment boundaries - followed by [recorded sweeps, used[0..K-1]].
 * hml_pool_export fills a device buffer of hml_pool_payload_size elements, hml_pool_install makes a (summed) payload
 * the context's marginals: hml_marginals_rle, hml_max_segmentation, hml_marginals_dense_device and hml_recorded_sweeps
 * then describe the pooled chains.  Any transport may sum the payloads in between. */
int hml_pool_payload_size(hml_ctx* ctx, uint64_t* n_int32);
int hml_pool_export(hml_ctx* ctx, void* payload_dev, int32_t* perm_out_or_null);
int hml_pool_install(hml_ctx* ctx, const void* payload_dev);
/* RCCL transport, one process per GPU: rank 0 creates the id (ncclGetUniqueId) and the launcher hands its
 * HML_POOL_ID_BYTES bytes to every rank; hml_pool_create is ncclCommInitRank (collective).  hml_pool_marginals =
 * export + ncclAllReduce(sum, int32) on the pool's stream + install (collective; every rank ends with the same
 * pooled marginals).  RCCL is loaded on the first of these calls (librccl.so.1). */
typedef struct hml_pool hml_pool;
#define HML_POOL_ID_BYTES 128
int hml_pool_unique_id(void* id /*HML_POOL_ID_BYTES*/);
int hml_pool_create(hml_pool** out, int device, int rank, int n_ranks, const void* id);
void hml_pool_destroy(hml_pool* pool);
int hml_pool_marginals(hml_pool* pool, hml_ctx* ctx, int32_t* perm_out_or_null);
int hml_pool_info(hml_pool* pool, int* rank, int* n_ranks, double* last_allreduce_ms, uint64_t* last_bytes, int* rccl_version);
/* The collective of hml_pool_marginals has two forms with the same result.  DENSE: the payload above through
 * ncclAllReduce(sum) - 4 (K+1)(T+1) bytes whatever it holds (2.4 GB at 10^8 positions and 5 states).  LISTS: the difference
 * arrays are zero except at recorded segment boundaries, so every rank sends the list of its marginal segments - header
 * [M, recorded sweeps, used[0..K-1]], then M x [position, relabelled deltas 0..K-1] - through ncclAllGather and adds all
 * lists into zeroed arrays (config 3 after 100 recorded sweeps: 23 000 segments, 0.6 MB per rank).  form 0 (default): the
 * lists when the gathered slots are at most an eighth of the dense payload - every rank decides alike from a handshake
 * that carries the ranks' segment counts; 1: always dense; 2: always lists.  Environment: HML_POOL_FORM.  The form is part
 * of the handshake: when the ranks hold different ones hml_pool_marginals returns HML_ERR_ARG on ALL of them.
 * hml_pool_last: the form the last call took (1 / 2) and, for the lists, the slot size in segments. */
int hml_pool_set_form(hml_pool* pool, int form);
int hml_pool_last(hml_pool* pool, int* form, uint64_t* entries);
/* One process driving n chains, e.g. one per GPU (`hammlet -chains N`): contexts sharing a device are summed there,
 * the per-device sums go through one grouped ncclAllReduce (ncclCommInitAll over the distinct devices), every context
 * receives the pooled marginals. */
int hml_allreduce_marginals(hml_ctx* const* ctxs, int n);
/* The same with the relabelling it applied: perms[i * K + j] = chain i's own label of pooled state j (may be null).  Chains
 * that all share one device are summed on it without RCCL. */
int hml_allreduce_marginals_perm(hml_ctx* const* ctxs, int n, int32_t* perms /* n * K */);
/* LABEL SPACES.  Pooling puts the context's MARGINALS (hml_marginals_rle, hml_max_segmentation, hml_marginals_dense_device)
 * into the common labels - states by ascending mean - while its parameters, state sequences and transition counts keep the
 * chain's own labels: perm[j] = the chain's label of pooled state j (the identity before any pooling).  A pooled context
 * refuses a second pooling (it would relabel and count twice) and refuses to record further sweeps into its marginals. */
int hml_pool_permutation(hml_ctx* ctx, int32_t* perm /*K*/);

/* ---- counters for measurement ---- */
typedef struct {
    uint64_t sweeps;            /* Gibbs sweeps executed                                   */
    uint64_t block_updates;     /* sum over sweeps of the number of blocks                 */
    uint64_t uniform_fallbacks; /* "[WARNING] Uniform sampling of forward variables!" count */
    uint64_t forward_refits;    /* chunks whose speculative forward pass had to be redone  */
    uint64_t forward_serial;    /* chunks finished by the sequential fallback              */
    uint64_t forward_warmup;     /* current (adaptive) warm-up length of the speculative forward pass */
    uint64_t fused_fallbacks;    /* tile words of the fused block kernel computed by a waiting workgroup (bounded wait expired) */
    uint64_t buffer_growths;     /* times the per-block buffers were grown (option "max_blocks", attached contexts) */
    uint64_t block_capacity;     /* blocks per sweep the per-block buffers hold at present */
} hml_stats;
int hml_get_stats(hml_ctx* ctx, hml_stats* out);

/* HIP-event timing of one named kernel family accumulated since the last reset (milliseconds and
 * launches); name is one of "blocks_compact", "blocks_scatter", "block_stats", "stats_emission", "emission", "forward",
 * "backward_maps", "backward_chain", "mixture", "counts", "params", "marginals", "levels", "breaks", "bands", "regions" (and inside it "regions_chunks", "regions_scan", "regions_accumulate"), "event_null".  level 0 = off, 1 = only the dominant kernel
 * ("blocks_compact", two events per sweep), 2 = every family. */
int hml_profile_enable(hml_ctx* ctx, int level);
int hml_profile_get(hml_ctx* ctx, const char* name, double* total_ms, uint64_t* launches);

/* parity probe for the arithmetic shared between the kernels and the CPU checker (hml_math.h, hml_dist.h):
 * evaluates function `fn` elementwise on the GPU (0 expf, 1 logf, 2 pow(a,b) on (0,1], 3 sqrtf, 4 a/b,
 * 5 gamma(alpha=a, beta=b) draw, 6 normal(mean=a, sd=b) draw, 7-10 double-precision kernels). */
int hml_debug_eval(int device, int fn, const float* a, const float* b_or_null, float* out, uint64_t n, uint64_t seed);

/* Device memory the library's contexts and read-outs hold at this moment, over the whole process: bytes and number of
 * allocations.  Both are 0 once every context, pooling object (hml_pool_create) and text reader is destroyed (and without a
 * GPU). */
int hml_device_memory_live(uint64_t* bytes, uint64_t* allocations);

/* Test hook for the out-of-memory paths: the `nth` device allocation from now (1: the next) fails once with
 * hipErrorOutOfMemory - the call that made it returns HML_ERR_HIP - without the runtime being asked, then the hook is off again;
 * 0 turns it off.  Returns the number of allocations made since the hook was last set.  Process-wide, like the totals above. */
int hml_debug_fail_allocation(int64_t nth);

/* Test mode for stores outside an array and reads of memory nobody wrote.  From the next allocation on
 * every device allocation of the library is guard + bytes + guard: both guards hold a fixed byte pattern, and with `poison`
 * the body is filled with 0xFF bytes (NaN as float or double, -1 or the maximum as an integer) before the allocation is
 * handed out.  `guard_bytes` is rounded up to a multiple of 256; 0 turns the mode off (allocations made under it stay
 * registered until they are freed).  Arming it restarts the count of allocations hml_debug_fail_allocation returns.
 * HML_GUARD_BYTES / HML_POISON in the environment arm it when the library is loaded.  Off by default; needs no device. */
int hml_debug_guard_allocations(uint64_t guard_bytes, int poison);

/* Waits for the devices of the registered allocations and reads their guards back.  *damaged: allocations found with a
 * damaged guard since the last reset, here or when they were freed (a free checks the buffer it frees).  For the first of
 * them: its ordinal among the allocations since the mode was armed (1: the first), the bytes its owner asked for, the side
 * (0: the guard before the body, 1: the one behind it) and the offset of the first damaged byte from that guard's start.
 * Any output may be null.  reset != 0 empties the report.  Each damaged allocation also prints one line to stderr that starts
 * with HML_GUARD_TAG.  Answers 0 damaged without a device. */
#define HML_GUARD_TAG "hml-guard:"
int hml_debug_check_guards(int reset, uint64_t* damaged, int64_t* ordinal, uint64_t* bytes, int* side, uint64_t* offset);

/* Proves from the host that the mode detects: a guarded, poisoned allocation reads back as 0xFF; one byte set just behind it
 * is reported by the check (side 1, offset 0, its size), one byte set just before it by the free of the buffer (side 0, the
 * guard's last byte).  Touches only memory the library owns; leaves the mode and the report as they were.  HML_ERR_HIP without
 * a device, HML_ERR_ARG with a message if the mode missed something or the report was not empty.  A test hook like the two
 * above: it sets and restores the mode's switches and the allocation count one after the other, so it must not run while another
 * thread allocates or frees device memory, and - like arming the mode - it makes a pending hml_debug_fail_allocation(nth) refer
 * to another allocation: set that hook afterwards. */
int hml_debug_guard_selftest(void);

/* synthetic piecewise-constant Gaussian trace, host buffer */
int hml_synth_gauss(float* x, int16_t* states_or_null, uint64_t T, int K, const float* mu, float sigma,
                    double mean_dwell, uint64_t seed, int nthreads);

/* simulated read-depth trace: copy-number segments, Poisson-lognormal counts as floats */
int hml_synth_depth(float* x, int16_t* states_or_null, uint64_t T, double depth, double ln_sigma, uint64_t seed, int nthreads);

#ifdef __cplusplus
}
#endif
#endif

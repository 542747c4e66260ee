// The chain context behind `hml_ctx*` (include/hml.h), shared by the translation units of libhammlet_hip.so
// (hml_capi.hip: the chain; hml_pool.hip: chain-parallel pooling over RCCL).
#ifndef HML_CTX_HPP
#define HML_CTX_HPP

#include <hip/hip_runtime.h>

#include <atomic>
#include <map>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "../../include/hml.h"
#include "hml_host_common.hpp"
#include "hml_layouts.h"
#include "hml_state.h"
#include "hml_sweep_plan.h"

// The read-only construction of one observation trace on one device - breakpoint weights, their group summary, maxlet
// coefficients, integral array(s) - shared by every chain that was attached to it (hml_attach_observations): the chains of a
// run read the same trace, their block sets are nested by threshold, and private copies (0.8 GB of integral array per chain at
// 10^8 positions) only defeat the caches.  Freed with the last context that holds it (hml_ctx::trace).
struct hml_trace {
    DevArr<float> d_w;
    DevArr<uint8_t> d_summary;
    DevArr<float> d_coeff;
    DevArr<float2> d_ia;
};

struct ProfAcc { double ms = 0; uint64_t n = 0; uint32_t tick = 0; std::vector<std::pair<hipEvent_t, hipEvent_t>> pending; };

// One per-position posterior summary that a recorded sweep accumulates beside the state marginals: emission levels, breakpoint
// counts, level bands.  All three keep difference arrays touched only where a run starts and a boundary bitmap of their own;
// what differs between them is in hml_recorder_kinds (hml_capi_shared.hpp).
enum { HML_REC_LEVELS = 0, HML_REC_BREAKS = 1, HML_REC_BANDS = 2, HML_REC_KINDS = 3 };
struct hml_recorder {
    bool on = false;                  // recording now (hml_set_level_recording / hml_set_break_recording / hml_set_level_bands; HML_LEVELS / HML_BREAKS / HML_BANDS)
    bool asked = false;               // ... was on at some time: the read-outs answer
    DevBuf d_acc;                     // [rows][T + 1] accumulators
    DevArr<uint32_t> d_boundary;      // its own bitmap of the positions with a cell
    template <class E> E* acc() const { return d_acc.as<E>(); }
};

// The joint posteriors over caller-given regions (hml_set_regions; hml_k_regions.h).  Not a fourth hml_recorder: no cells per
// position and no bitmap, a few words per region instead.
struct hml_regions {
    bool on = false;                  // recording now
    bool asked = false;               // ... was on at some time: the read-out answers
    bool checked = false;             // the regions were compared with T (at hml_set_regions, or at the first recorded sweep)
    std::vector<uint32_t> start, end; // the regions last set, [start, end) each (they stay when the recording is turned off)
    int n_edges = 0;                  // the regions' own band edges (0: no band columns)
    float edges[31] = {};
    DevArr<uint32_t> d_start, d_end;
    DevBuf d_acc;                     // the accumulators of hml_regions_acc, one allocation
    DevBuf d_chunks;                  // chunk totals of a recorded sweep, sized by T (hml_regions_chunks)
};

// The chain's history (hml_set_history; hml_k_history.h): a row of scalars per due sweep, written on the device behind the
// sweep's parameter update.  The host sizes the buffer ahead of the sweeps it enqueues and never looks at it in between.
struct hml_history {
    bool on = false;                  // sweeps launch the history kernel
    uint64_t every = 1;               // a sweep is due when the chain's sweep counter is a multiple of it
    DevBuf d_buf;                     // hml_history_head, then `cap` rows of HML_HISTORY_COLS doubles
    uint64_t cap = 0;                 // rows the buffer holds
    uint64_t expected = 0;            // rows it holds once everything enqueued has run (never less than that)
    uint64_t grown = 0;               // times it was replaced by a larger one
};

struct hml_ktab;   // hml_capi_shared.hpp

struct hml_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    uint64_t seed = 0;
    uint32_t chain = 0;
    uint64_t T = 0;
    int K = 0;
    int D = 1, P = 0;              // data dimensions / emission parameters ("-s C P D"; P = 0: univariate, P = K)
    bool loaded = false, model_set = false;
    bool dynamic = true;
    bool blocks_valid = false;     // starts/bstat describe the current threshold
    double sigma = 0;
    // construction (owned by `trace`, which the contexts attached to it share; the pointers below are this context's view of it)
    std::shared_ptr<hml_trace> trace;
    float* d_w = nullptr;
    uint8_t* d_summary = nullptr;  // largest key of every 16-position group (what the scan streams)
    int32_t key_base = 0;
    double key_scale = 1.0;         // product of the weight multipliers applied so far
    uint64_t host_draws = 0;        // hml_categorical_draw calls so far (Philox sub-stream HOST)
    float* d_coeff = nullptr;
    float2* d_ia = nullptr;
    // block structure
    DevArr<uint16_t> d_stage;
    DevArr<uint32_t> d_span_count, d_starts;
    DevArr<float2> d_bstat;
    uint32_t n_spans = 0;
    DevArr<uint32_t> d_coarse1;      // block count per group of HML_GROUP_SPANS spans
    DevArr<unsigned long long> d_group_word;      // fused block kernel: {generation, starts, last start} per tile
    DevArr<uint32_t> d_wave_total;                // split many-chain block kernels: starts per wavefront of a tile (hml_k_blocks_split_many.h)
    int fused_slots = 0;                          // workgroups of it that are resident at once (occupancy x compute units; 0: not asked yet)
    uint32_t fused_spin_limit = 4096;             // polls of a tile word before the waiting thread computes the word itself
    DevArr<unsigned long long> d_dbg;             // HML_FUSED_DEBUG: the block kernels' time stamps (hml_sync prints them)
    hml_sweep_knobs knobs;          // what steers which kernels a sweep launches (hml_sweep_plan.h)
    // hipGraph replay of a non-recording sweep (launch-bound inner loop); re-captured when the plan or the grid hint moves
    bool use_graph = false;
    hipGraphExec_t graph_exec = nullptr;
    struct { hml_sweep_plan plan; uint32_t hint = 0, tre_L = 0; } captured;   // what the captured sweep was recorded under
    // sweep buffers (allocated by set_model)
    DevArr<float> d_em, d_gsc, d_rows, d_eprobe, d_aprobe;
    DevArr<float> d_entry, d_exitA;
    DevArr<uint32_t> d_redo;       // backward chunks that failed the forward verification (list for the repair step)
    DevArr<uint32_t> d_redo2;      // second list of stale chunks and the bitmap of the sequential finisher (fused trellis path)
    DevArr<uint32_t> d_tre_bitmap;
    DevArr<uint32_t> d_tre_ckpt;         // the first pass's forward vectors every 64 rows of a chunk (hml_k_trellis_rows.h): where a refit may stop
    uint32_t tre_L = 0;            // its chunk length (0: chosen from the number of blocks, then by measurement; HML_TRELLIS_L, option "trellis_L")
    // The best chunk length depends on how the wavefronts of hml_k_trellis_tile (64 chunks each, resident for the whole
    // launch) divide among the CUs' slots - a rounding effect no formula of ours predicted - so it is MEASURED: once the
    // warm-up policy has settled, every candidate length runs two sweeps between a pair of events and the fastest
    // stays.  The chain's results do not depend on the chunk length (rows, maps and draws are addressed by block).
    bool tre_autotune = true;      // HML_TRELLIS_TUNE=0: keep the length chosen from the number of blocks
    uint32_t tre_tuned_L = 0, tre_tuned_hint = 0;
    int tre_tune_step = -1;        // >= 0 while measuring: candidate step % n, pass step / n
    float tre_tune_ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t tre_cand[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // the candidate lengths of the measurement under way (frozen when it starts:
    int tre_cand_n = 0;                               // the list depends on the drifting block count)
    uint64_t tre_dense_sweeps = 0; // fused-trellis sweeps of this chain so far
    uint32_t tre_last_L = 0;       // chunk length of the latest fused-trellis sweep
    int tre_slots = 0;             // wavefronts of hml_k_trellis_rows the device holds at once (0: not asked yet, -1: unknown)
    uint32_t tre_refit_rounds = 2; // parallel refit rounds before the sequential finisher (HML_TRELLIS_REFIT_ROUNDS, 0 ... 6: the rounds tag the chunks they list with 3 bits).
                                   // Four until the end of round 5: on configs 3u and 5 rounds 2-4 never had a chunk to refit in 240 sweeps and cost 9 us each
                                   // (two launches at the 4.6 us floor of a kernel in a stream; profiles/round5_refit_rounds.txt)
    bool tre_ckpt = true;          // refits stop where they meet the first pass's checkpoint again (HML_TRELLIS_CKPT=0: always the whole chunk)
    DevArr<uint32_t> d_touched;    // backward chunks whose rows the repair recomputed, tagged with the sweep
    DevArr<uint32_t> d_fb;
    DevArr<unsigned long long> d_smap, d_cmap;
    DevArr<unsigned long long> d_scmap, d_super;   // two-level chain (weakly compressed sweeps)
    DevArr<uint8_t> d_bentry, d_bentry2;
    DevArr<int16_t> d_q;
    DevArr<double> d_partial;
    DevArr<int32_t> d_diff;
    DevArr<uint32_t> d_boundary;
    // the per-position recordings beside the state marginals (hml_recorder above), allocated by the first recorded sweep that wants them:
    //   HML_REC_LEVELS  double [2 D][T + 1]: row 2 d the level's difference array, row 2 d + 1 its square's (hml_k_levels.h);
    //                   nothing recorded: one segment, zero sums
    //   HML_REC_BREAKS  uint32 [T + 1]: recorded sweeps with a breakpoint at t (hml_k_breaks.h); nothing recorded: an empty list
    //   HML_REC_BANDS   int32 [D (n_band_edges + 1)][T + 1]: difference arrays of the counts per band (hml_k_bands.h);
    //                   nothing recorded: one segment of zeros
    hml_recorder rec[HML_REC_KINDS];
    hml_regions rg;
    hml_history hist;
    int n_band_edges = 0;           // the bands' edges last set (they stay when the recording is turned off)
    float band_edges[31] = {};
    DevArr<hml_model> d_mdl;
    uint32_t* h_B = nullptr;       // pinned + mapped, four words: [0] the block count of the latest enumeration (grid sizing hint),
                                    // [1] set by the fused block kernel when a bounded wait expired, [2] the chain is HALTED: the number of
                                    // blocks an enumeration found beyond the capacity of the per-block buffers (hml_state.h)
    // Block capacity of the per-block buffers (0 until the observations are loaded; T = the worst case, every position a block).
    // Less for a context with option "max_blocks" and, by default, for a context ATTACHED to another one's observations; a sweep
    // that needs more halts the chain on the device, and the host grows the buffers and runs the missing sweeps again
    // (hml_settle) - `sweep_log` holds what was enqueued since the last point at which the stream was known to be idle.
    uint64_t cap = 0;
    uint64_t cap_opt = 0;           // option "max_blocks" / HML_MAX_BLOCKS (0: the default of the context's kind)
    std::vector<uint8_t> sweep_log; // per enqueued sweep: bit 0 mixture, bit 1 recorded
    unsigned long long log_base = 0;   // the model's sweep counter when the log started (= sweeps requested up to then)
    unsigned long long requested = 0;  // sweeps requested of this chain so far (its sweep counter once everything has run)
    unsigned long long call_base = 0;  // `requested` when the current hml_iterate / hml_iterate_many call began: a sweep's index in
                                       // its call (what the recording callback is told) = its ordinal - call_base
    uint64_t grown = 0;             // times the buffers were grown (hml_stats)
    uint32_t* d_hB = nullptr;       // device view of h_B (not an allocation of its own)
    uint32_t B_hint = 0;
    bool hint_stale = true;         // the hint predates the current parameters (new model, prior draw, mode switch)
    // warm-up of the forward chunks (their lengths and layouts: knobs.geo)
    int fwdW = 12;   // W is the floor of the adaptive warm-up (measured: 12 beats 16 and 24 on C1-C4; 8 does not)
    // the warm-up policy of hml_k_params (HML_FWD_BURNIN_SWEEPS, HML_FWD_QUIET): the floor of a young chain holds for 64
    // sweeps and the warm-up shrinks by a quarter after 16 sweeps without a refit.  Measured over the first 400 sweeps
    // of configs 2 / 3 / 4 (tools/burnin_sweep.sh): 19.9 / 25.4 / 50.4 ms against 21.0 / 26.1 / 52.2 ms with (256, 32);
    // (32, 8) and faster let the warm-up fall while the parameters still move - bursts of 150+ refits, 26.6 ms on config 3
    uint32_t fwd_burnin_sweeps = 64, fwd_quiet_need = 16;
    int fwdW_init = 24;        // where a chain starts and the floor of its first fwd_burnin_sweeps sweeps: while the parameters are
                               // still far from settled the filter forgets slowly (131 refits in sweeps 20-220 of C3 with a floor of 12)
    bool probes = false;
    bool rec_marginals = true;
    hml_record_cb cb = nullptr;
    void* cb_user = nullptr;
    int fm_slots = 0;              // workgroups of the many-chain block kernel that are resident at once (0: not asked yet)
    DevBuf d_many;                 // hml_iterate_many: the chains' pointers (hml_chain_dev), kept by the first chain of a batch
    int many_cap = 0;
    bool compat = false;           // option "compat": sweeps exactly as the reference computes them (hml_k_compat.h)
    DevBuf d_mt;                   // its engine (hml_mt_state)
    DevArr<float> d_crows;         // its trellis, (T + 1) x K
    DevBuf d_cchunk;               // chunks of its filter / backward draws (hml_compat_chunks, hml_k_compat.h)
    DevArr<uint32_t> d_cdraws;     // the engine's outputs of a sweep's categorical draws
    DevBuf d_clists;               // its count pass's lists by state (hml_compat_lists)
    hml_rtk_knobs rtk;             // what steers the sweeps of the two paths that take the number of states at run time (hml_rtk_plan.h)
    const hml_ktab* kt = nullptr;  // the sweep, parameter and allocation functions of the context's path (hml_set_model; hml_capi_shared.hpp)
    bool wide = false;            // more than 16 states on the default path: the number of states is a run-time value, a state a lane (hml_k_wide.h)
    DevBuf d_wacc;                 // its integer counts of a sweep (hml_wide_acc)
    DevArr<float> d_wA;            // ... the transition matrix padded to 64 x 64 (hml_k_wide_lanes.h)
    bool pooled = false;           // the marginals are a pooled payload (hml_pool_install): common labels, counts of several chains
    std::vector<int32_t> pool_perm;   // perm[pooled label] = this chain's label, from the export that preceded the pooling
    int profiling = 0;             // 0 off, 1 dominant kernel only (blocks_compact, every 32nd launch), 2 every kernel family
    uint32_t prof_tick = 0;
    std::map<std::string, ProfAcc> prof;
    std::vector<hipEvent_t> ev_pool;
    // A chunked pass over the blocks under the current parameters (hml_infer.hip).  Launch geometry only, and what the last
    // call did.  Its device memory lives for the length of a call.
    struct chunked_pass {
        uint32_t W = 0, L = 0;         // warm-up and chunk length in blocks (0: the defaults)
        uint32_t rounds = 8;           // parallel repair rounds before the single lane
        bool done = false;             // a call has run: the numbers below are its
        uint64_t chunks = 0, used_L = 0, used_W = 0, stale[2] = {0, 0}, rounds_run = 0, walked = 0;   // stale: forward, backward
    };
    // The Viterbi decode (hml_viterbi; hml_k_viterbi.h): options "viterbi_W", "viterbi_L", "viterbi_rounds"; hml_viterbi_info.
    // It has one direction: stale[0].
    chunked_pass vit;
    // Smoothing (hml_posterior; hml_k_posterior.h): options "posterior_W", "posterior_L", "posterior_rounds"; hml_posterior_info.
    chunked_pass post;
    // EM from many starts (hml_em_fit_many; hml_k_em_many.h): the byte budget of a group's device memory (0: the default) and what
    // the last call did (hml_em_many_info).
    struct {
        uint64_t batch_bytes = 0;
        bool computed = false;
        uint64_t members = 0, groups = 0, group_size = 0, esteps = 0, launch_sets = 0, stale_fwd = 0, stale_bwd = 0, rounds_run = 0, walked = 0;
    } em_many;
    // Sampled paths (hml_posterior_sample; hml_k_sample.h): options "sample_W", "sample_L", "sample_rounds"; the byte budget of a
    // group of draws (0: the default) and what the last call did (hml_posterior_sample_info).  stale[0] and walked: over all groups.
    chunked_pass samp;
    struct {
        uint64_t batch_bytes = 0, draws = 0, groups = 0, group_size = 0;
    } samp_batch;
    // Count read-outs (hml_posterior_region_counts; hml_k_counts.h): what the last call did (hml_posterior_counts_info).
    struct {
        bool done = false;
        uint64_t regions = 0, steps = 0, longest = 0;   // steps: the sum of be - ba over the regions; longest: the largest
    } counts;
    // Every d_* above that is not a plain pointer owns its buffer (DevBuf / DevArr, hml_host_common.hpp): deleting the context
    // frees them, whatever a call that failed half-way left allocated, and allocating one again replaces what it held.
    ~hml_ctx() { if (h_B) (void)hipHostFree(h_B); }
};

// hml_capi.hip
int hml_ctx_bind(hml_ctx* c);                         // hipSetDevice(ctx's device)
int hml_ctx_fetch_model(hml_ctx* c, hml_model* out);  // synchronising copy of the device-resident model
int hml_ctx_ensure_marginal_buffers(hml_ctx* c);
int hml_settle(hml_ctx* c);                           // stream idle, no halted sweep left behind (block capacity, above)
// hml_readout.hip (hml_infer.hip, the library's other read-out object, declares nothing here: it is reached through the C ABI alone)
// marginal segments on the device: starts d_seg[M] and count differences at the starts d_g[M * K]
int hml_ctx_gather_marginal_segments(hml_ctx* c, uint64_t* M, DevBuf& d_seg, DevBuf& d_g);

#endif

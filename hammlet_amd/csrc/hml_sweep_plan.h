// What a sweep of the default path launches, decided in ONE place: the settings that steer the choice (hml_sweep_knobs, a
// member of hml_ctx), the choice itself (hml_sweep_plan) and the pure function between them (hml_plan_sweep).  No HIP in
// here: a host compiler alone builds it (tests/test_sweep_plan_cpu.py).  sweep_k (hml_sweep.hip) computes the plan of a sweep
// from its first read of the block-count hint and launches from it; hml_iterate compares the plan of the coming sweep
// with the one its captured graph was recorded under.  Which plan a sweep runs under never changes its results.
#ifndef HML_SWEEP_PLAN_H
#define HML_SWEEP_PLAN_H

#include <stdint.h>

#include "hml_state.h"

// the four forward geometries: a chunk length and the chunk-transposed layout of that length (hml_state.h)
enum { HML_GEO_SPARSE = 0, HML_GEO_MID = 1, HML_GEO_DENSE = 2, HML_GEO_MANY = 3, HML_GEO_KINDS = 4 };
struct hml_fwd_geo { int L; hml_layout lay; };

struct hml_sweep_knobs {
    // forward geometry: chunks of 4 (sparse), and - dense:
    // weakly compressed sweeps (B_hint >= dense_min_blocks): longer forward chunks - the warm-up is a smaller share
    // of the work - in their own chunk-transposed layout; which geometry a sweep uses never changes its results
    // mid: in between (B_hint >= mid_min_blocks = 2^18: 33 000 chunks of 8 still put a wavefront on every second SIMD): chunks of 8 - 32 filter
    // steps per 8 blocks instead of 28 per 4.  Measured on config 3's trace with 8 / 10 / 12 / 16 states in the model (3.0 / 5.2 / 7.2 /
    // 9.7 10^5 blocks per sweep): 0.188 / 0.228 / 0.489 / 0.498 -> 0.165 / 0.224 / 0.429 / 0.437 ms per sweep; with 5 states (1.8 10^5 blocks:
    // below the threshold) chunks of 8 cost 0.063 against 0.060 ms (profiles/round5_wide_path.txt).  HML_FWD_CHUNK_MID, HML_MID_MIN_BLOCKS.
    // many: chains batched by hml_iterate_many are bound by throughput, not latency: chunks of 8 pay the warm-up over twice as many
    // blocks (20 filter steps per 8 blocks instead of 16 per 4; measured with eight chains of config 3: 0.181 against 0.188 ms
    // per round; 16 and 32 are slower again - too few wavefronts).  HML_FWD_CHUNK_MANY.
    hml_fwd_geo geo[HML_GEO_KINDS] = {{4, {2, 0}}, {8, {3, 0}}, {16, {4, 0}}, {8, {3, 0}}};   // sparse, mid, dense, many
    uint32_t mid_min_blocks = 1u << 18;
    uint32_t dense_min_blocks = 1u << 22;
    bool late_rescale = true;      // strongly compressed univariate sweeps: no plane of rescale factors (HML_LATE_RESCALE=0: keep it)
    bool tre_fused = true;         // weakly compressed FB sweeps take the fused trellis kernels (HML_TRELLIS_FUSED=0: the separate ones)
    bool tre_rows = true;          // its first pass is hml_k_trellis_rows (round 3); HML_TRELLIS_ROWS=0: hml_k_trellis_tile (round 2)
    bool use_keys = true;
    bool summary_always = false;    // option weight_keys = 2: never fall back to the float stream (tests)
    bool stage_bits = true;        // weakly compressed sweeps stage block-start FLAGS between scan and scatter (HML_STAGE_BITS=0: 16-bit offsets)
    bool fused_blocks = true;       // option fused_blocks: 0 forces the scan + scatter + statistics launches
    bool fused_keep = false;                      // option fused_blocks = 2 (tests): keep the kernel after it reported trouble
    bool params_spread = false;    // single-chain sweeps: the parameter kernel's tree over 16 workgroups (hml_k_params.h; HML_PARAMS_SPREAD)
};

enum { HML_SCAN_SUMMARY = 0, HML_SCAN_FLOAT = 1, HML_SCAN_FLAGS = 2 };           // first launch of the scan + scatter pair
enum { HML_PASS_ROWS_SINGLE = 0, HML_PASS_ROWS = 1, HML_PASS_TILE = 2 };         // hml_k_trellis_rows<K, true> / <K, false> / hml_k_trellis_tile
enum { HML_COUNTS_MV = 0, HML_COUNTS_DENSE = 1, HML_COUNTS_PLAIN = 2 };          // hml_k_counts<.., true> / hml_k_counts_dense / hml_k_counts

struct hml_sweep_plan {
    uint8_t geo = HML_GEO_SPARSE;   // index of the forward geometry, with its chunk length and layout
    int L = 0;
    hml_layout lay = {0, 0};
    bool mix = false;               // a mixture sweep (no filter, no maps)
    bool many_blocks = false;       // hml_plan_many_blocks: the backward chain in two levels
    bool float_stream = false;      // hml_plan_float_stream
    bool keep_gsc = true;           // the plane of rescale factors is kept
    bool trellis = false;           // emission terms, filter and candidate maps fused per tile (hml_k_trellis.h)
    bool fused_wanted = false;      // the fused block kernel, if its tile fits the resident grid (sweep_k); else scan + scatter
    uint8_t scan = HML_SCAN_SUMMARY;
    uint8_t first_pass = HML_PASS_TILE;
    uint8_t counts = HML_COUNTS_PLAIN;
    bool params_spread = false;
};
static inline bool operator==(const hml_sweep_plan& a, const hml_sweep_plan& b) {
    return a.geo == b.geo && a.L == b.L && a.lay.lshift == b.lay.lshift && a.lay.cstride == b.lay.cstride && a.mix == b.mix &&
           a.many_blocks == b.many_blocks && a.float_stream == b.float_stream && a.keep_gsc == b.keep_gsc && a.trellis == b.trellis &&
           a.fused_wanted == b.fused_wanted && a.scan == b.scan && a.first_pass == b.first_pass && a.counts == b.counts &&
           a.params_spread == b.params_spread;
}

// `hint` is the block count of an earlier sweep with its headroom (hml_ctx::B_hint), 0 while none is known.
static inline bool hml_plan_many_blocks(const hml_sweep_knobs& k, uint32_t hint) { return hint >= k.dense_min_blocks; }
// the summary scan skips unopened groups; when most groups would be opened (weak compression) the plain
// float stream is the better access pattern - both give the same blocks
static inline bool hml_plan_float_stream(const hml_sweep_knobs& k, uint64_t T, uint32_t hint) {
    return !k.summary_always && hint != 0u && (uint64_t)hint * 24u > T;
}
// ... and with B ~ T the scan stages the flags themselves (512 bytes per span) instead of 16-bit offsets (2 bytes per block)
static inline uint8_t hml_plan_scan(const hml_sweep_knobs& k, uint64_t T, uint32_t hint) {
    const bool fs = hml_plan_float_stream(k, T, hint);
    return (k.use_keys && !fs) ? HML_SCAN_SUMMARY : (fs && k.stage_bits) ? HML_SCAN_FLAGS : HML_SCAN_FLOAT;
}

// alone_on_device: no other live context on the chain's device; wait_expired: a bounded wait of the fused block kernel expired
static inline hml_sweep_plan hml_plan_sweep(const hml_sweep_knobs& k, uint64_t T, int D, bool mix, uint32_t hint, bool alone_on_device, bool wait_expired) {
    hml_sweep_plan p;
    p.mix = mix;
    p.many_blocks = hml_plan_many_blocks(k, hint);
    p.float_stream = hml_plan_float_stream(k, T, hint);
    // weakly compressed univariate FB sweeps: emission terms, filter and candidate maps fused per tile (hml_k_trellis.h)
    p.trellis = p.many_blocks && !mix && D == 1 && k.tre_fused;
    const bool mid = !p.many_blocks && k.geo[HML_GEO_MID].L > k.geo[HML_GEO_SPARSE].L && hint >= k.mid_min_blocks;   // (chunks of 8 from 2^18 blocks on)
    p.geo = p.many_blocks ? HML_GEO_DENSE : mid ? HML_GEO_MID : HML_GEO_SPARSE;
    p.L = k.geo[p.geo].L;
    p.lay = k.geo[p.geo].lay;
    // strongly compressed univariate sweeps keep no plane of rescale factors: the forward rows stay unscaled and the
    // backward maps apply the factor where they read a row (hml_bwd_row_load) - 3.5 of the block kernel's 11 MB of
    // stores at 10^8 positions, and what a dependent launch waits for is the write-back of its predecessor's stores
    p.keep_gsc = p.many_blocks || !k.late_rescale;
    // the fused block kernel: univariate chains that have the GPU to themselves, unless compression is weak (the
    // float stream is the better access pattern then) or the kernel reported a bounded wait that expired
    p.fused_wanted = D == 1 && k.use_keys && k.fused_blocks && !(wait_expired && !k.fused_keep) && alone_on_device && !p.float_stream;
    p.scan = hml_plan_scan(k, T, hint);
    // (nearly every block a single position: the filter step shares the candidate maps' sums, hml_k_trellis_rows.h)
    // (last sweep's blocks >= 0.9 T; the hint carries 25 % headroom)
    p.first_pass = (k.tre_rows && hint > 1024u && ((uint64_t)hint - 1024u) * 8u >= T * 9u) ? HML_PASS_ROWS_SINGLE : k.tre_rows ? HML_PASS_ROWS : HML_PASS_TILE;
    // many blocks: hundreds of chunks per workgroup, one wavefront per chunk (same tree, bit for bit)
    p.counts = D > 1 ? HML_COUNTS_MV : p.many_blocks ? HML_COUNTS_DENSE : HML_COUNTS_PLAIN;
    p.params_spread = k.params_spread;
    return p;
}

#endif

// What a sweep launches on the two paths that take the number of states at run time - the reference-compatible mode
// (hml_k_compat.h) and the path for more than 16 states (hml_k_wide.h, hml_k_wide_lanes.h) - decided in ONE place, like
// hml_sweep_plan.h for the default path: the settings (hml_rtk_knobs, a member of hml_ctx), the choice (hml_rtk_plan) and the
// pure function between them (hml_plan_rtk).  The sweeps (hml_rtk_sweep.hpp) compute the plan once from their first read of the
// block-count hint and launch from it; the buffers are sized from hml_plan_wl_geometry, which the plan uses too.  No HIP in
// here: a host compiler alone builds it (tests/test_rtk_plan_cpu.py).  Every chunk is verified bit for bit, so which plan a
// sweep runs under never changes its results.
#ifndef HML_RTK_PLAN_H
#define HML_RTK_PLAN_H

#include <stdint.h>

#include "hml_common.h"

#define HML_COMPAT_MAX_CHUNKS 16384   // (round 5: 2048 before - a chunk is one wavefront, and the machine holds 8000 of them)
#define HML_CHUNK_W_ADAPTIVE 0xffffffffu   // hml_compat_chunks::W: the model's own warm-up (hml_chunk_warmup, hml_k_compat.h)
#define HML_WL_MAX_CHUNKS 131072
#define HML_WL_MIN_LSHIFT 2
// the filter's registers let two wavefronts onto a SIMD up to this many (padded) states - up to 32 as the compiler allocates them, at
// 36 when told to and with the step's loads asked for behind the products (219 registers; 40 states fit too, 240 registers, and gain
// nothing; from 48 on the kernel would spill) - and a sweep is then cut into twice the chunks (hml_k_wl_prepare)
#define HML_WL_TWO_WAVES_KC 36

struct hml_rtk_knobs {
    int compat_chunks = 0;         // 0: chosen from the block count; 1: the sequential form (HML_COMPAT_CHUNKS)
    int compat_warmup = 0;         // blocks a chunk runs ahead of its first; 0: the model's adaptive one; < 0: none (HML_COMPAT_WARMUP)
    int wide_lanes = 1;            // more than 16 states: filter and backward draws with a chunk a lane (0: a state a lane, hml_k_compat.h's kernels) (HML_WIDE_LANES)
    int wide_w0 = 32;              // ... the floor of its chunks' adaptive warm-up, blocks (HML_WIDE_W0)
    uint32_t wide_max_chunks = 0;  // ... the most chunks a sweep is cut into (HML_WIDE_MAX_CHUNKS; 0: HML_WL_MAX_CHUNKS)
    int wide_lshift = -1;          // ... log2 of a forced chunk length (tests: HML_WIDE_L), -1: from the block count
};

// The chunk-a-lane path's geometry, as hml_k_wl_prepare is told it: the most chunks a sweep is cut into, and the shortest chunks
// it can choose.  The buffers are sized for the chunk lengths these give at the context's capacity (hml_layouts.h).
struct hml_wl_geometry { uint32_t max_chunks; uint32_t min_L; };
static inline hml_wl_geometry hml_plan_wl_geometry(const hml_rtk_knobs& k, int K) {
    hml_wl_geometry g;
    if (k.wide_max_chunks) g.max_chunks = k.wide_max_chunks < (uint32_t)HML_WL_MAX_CHUNKS ? k.wide_max_chunks : (uint32_t)HML_WL_MAX_CHUNKS;
    else g.max_chunks = K <= HML_WL_TWO_WAVES_KC ? (uint32_t)HML_WL_MAX_CHUNKS : (uint32_t)HML_WL_MAX_CHUNKS / 2u;
    g.min_L = 1u << (k.wide_lshift >= 0 ? k.wide_lshift : HML_WL_MIN_LSHIFT);
    return g;
}

enum { HML_RTK_COMPAT = 0, HML_RTK_WIDE = 1 };                              // the mode
enum { HML_RTK_SEQUENTIAL = 0, HML_RTK_CHUNKED = 1, HML_RTK_LANES = 2 };    // a state a lane in one chunk / in C chunks; a chunk a lane
enum { HML_RTK_EXP_GLIBC = 0, HML_RTK_EXP_DEV = 1 };                        // hml_glibc_exp / hml_dev_exp

struct hml_rtk_plan {
    uint8_t form = HML_RTK_SEQUENTIAL;   // of filter and backward draws (a mixture sweep has neither: `mix`)
    bool mix = false;
    uint32_t C = 1;                 // chunks of the state-a-lane forms (grid of hml_k_compat_forward / _backward)
    uint32_t W = HML_CHUNK_W_ADAPTIVE;   // hml_compat_chunks::W
    bool by_state = false;          // the count pass over lists by state (hml_k_compat_part_*), not in block order
    uint8_t exp = HML_RTK_EXP_GLIBC;
    int KC = 0;                     // the dispatch's bucket: K up to 16, then 32 or 64; chunk a lane: K rounded up to a multiple of 4
    bool pad = false;               // ... a state a lane: KC is an upper bound of the model's K, not K itself
    hml_wl_geometry wl = {0u, 0u};  // chunk a lane: what hml_k_wl_prepare is told ...
    uint64_t room = 0;              // ... and the blocks its grids are sized for (the kernels find B themselves)
};

// `hint` is the block count the sweep's grids are sized for (grid_hint); `probes`: the rows are probed (hml_enable_probes).
static inline hml_rtk_plan hml_plan_rtk(const hml_rtk_knobs& k, int mode, int K, int D, uint64_t T, bool mix, bool probes, uint32_t hint) {
    hml_rtk_plan p;
    const bool wide = mode == HML_RTK_WIDE;
    p.mix = mix;
    p.W = k.compat_warmup > 0 ? (uint32_t)k.compat_warmup : k.compat_warmup < 0 ? 0u : HML_CHUNK_W_ADAPTIVE;   // (< 0: none - tests)
    p.exp = wide ? HML_RTK_EXP_DEV : HML_RTK_EXP_GLIBC;
    // a chunk a lane over chunk-transposed arrays (hml_k_wide_lanes.h) - unless the rows are probed, a test asked for a number of
    // chunks of the other form, or the sweep has no filter at all
    if (wide && k.wide_lanes != 0 && !probes && !mix && k.compat_chunks == 0) {
        p.form = HML_RTK_LANES;
        p.KC = (K + 3) / 4 * 4;
        p.wl = hml_plan_wl_geometry(k, K);
        p.room = (uint64_t)hint + hint / 4 + 1024;
        return p;
    }
    // a state a lane, a wavefront per chunk; one chunk - the sequential form - for short sweeps and when the rows are probed
    // (a mixture sweep has no filter to cut)
    const bool chosen = k.compat_chunks == 0 && hint >= (wide ? 2048u : 8192u);
    const uint32_t most = HML_COMPAT_MAX_CHUNKS;
    if (probes || mix) p.C = 1u;
    else if (k.compat_chunks > 1) p.C = (uint32_t)k.compat_chunks < most ? (uint32_t)k.compat_chunks : most;   // (tests: any sweep in that many chunks)
    else if (chosen) p.C = hint / 64u < most ? hint / 64u : most;
    p.form = p.C > 1u ? HML_RTK_CHUNKED : HML_RTK_SEQUENTIAL;
    // (up to 16 states: the number of states as a compile-time value - A in registers, loops unrolled; beyond, and on the path for
    // more than 16 states: loops unrolled over 32 or 64 in groups of four that stop at the model's value)
    p.pad = wide || K > HML_MAX_K;
    p.KC = !p.pad ? K : K <= 32 ? 32 : 64;
    // the count pass by state for long univariate sweeps of the reference-compatible mode, whether probed or not (a block's size and
    // a flag share a word of the lists: traces below 2^31 positions)
    p.by_state = !wide && D == 1 && T < (1ull << 31) && (k.compat_chunks > 1 || chosen);
    return p;
}

#endif

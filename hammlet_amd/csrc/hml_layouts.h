// The device buffers that hold several arrays, each with ONE layout: a function that carves the buffer's arrays from a base
// pointer in order.  The allocation calls it on a null base for the byte count, the launch sites on the buffer for the views,
// so a change to an array cannot miss one of them.  No HIP in here: a host compiler alone builds it and a test walks the
// layouts over capacities and numbers of states (tests/test_layouts_cpu.py).
#ifndef HML_LAYOUTS_H
#define HML_LAYOUTS_H

#include <assert.h>
#include <stddef.h>
#include <stdint.h>

#include "hml_rtk_plan.h"

// Hands out arrays from `base` in order, each aligned to its element type or to what the layout asks for.  The base is taken
// to be aligned to 16 bytes (device allocations are, to 256); on a null base the pointers are offsets and bytes() the size.
class hml_carver {
    uintptr_t base_;
    uint64_t off_ = 0;
public:
    explicit hml_carver(void* base) : base_((uintptr_t)base) { assert((base_ & 15u) == 0u); }
    template <class E> E* take(uint64_t n, uint64_t align = alignof(E)) {
        assert(align >= alignof(E) && align <= 16u && (align & (align - 1u)) == 0u);
        off_ = (off_ + align - 1u) & ~(align - 1u);
        E* const p = (E*)(base_ + off_);   // (integer arithmetic: nothing here is dereferenced, and the base may be null)
        off_ += n * sizeof(E);
        return p;
    }
    void slack(uint64_t bytes) { off_ += bytes; }   // room behind the arrays that nothing points to
    uint64_t bytes() const { return off_; }
};

// ---- d_cchunk: the chunks of filter and backward draws of the two run-time-K paths (hml_k_compat.h: "in CHUNKS")
struct hml_compat_chunks {
    float* entry;        // [C][K] filter: the row a chunk reached at its first block (from its warm-up)
    float* exitv;        // [C][K] ... and the unscaled row it left behind its last block
    uint32_t* bad;       // [C] filter: the chunk's entry row is not what the chunk before it left (hml_k_compat_forward_verify)
    uint32_t* nfb;       // [C] uniform fallbacks inside the chunk's own blocks
    int32_t* in_state;   // [C] backward draws: the state above the chunk's first row (from its warm-up)
    int32_t* out_state;  // [C] ... and the state of its last row
    uint32_t W;          // warm-up, blocks; HML_CHUNK_W_ADAPTIVE: the model's own (mdl->fwd_W: it follows the chunks that had to run again)
    unsigned long long* tot;   // [3] (hml_k_wide_lanes.h) wrong chunks of the filter, the sum of nfb, wrong chunks of the backward draws
};
// hml_compat_chunks::tot on the chunk-a-lane path: [0] wrong chunks of the filter, [1] the sum of nfb, [2] wrong chunks of the backward draws,
// then a bit per wrong chunk of the filter and of the backward draws (set by the verifying launches, cleared by the checking ones)
#define HML_WL_MAP_WORDS (HML_WL_MAX_CHUNKS / 64)
#define HML_WL_MAP_F 4
#define HML_WL_MAP_B (HML_WL_MAP_F + HML_WL_MAP_WORDS)
#define HML_WL_TOT_WORDS (HML_WL_MAP_B + HML_WL_MAP_WORDS)
#define HML_COMPAT_TOT_WORDS 8   // the reference-compatible mode: the three counters, in 64 bytes behind the arrays
static_assert(HML_COMPAT_TOT_WORDS >= 3 && HML_WL_TOT_WORDS >= HML_WL_MAP_B + HML_WL_MAP_WORDS, "tot holds its counters (and, a chunk a lane, both bit maps)");

// chunks the arrays hold.  Reference-compatible mode: the most a sweep is cut into.  More than 16 states: as many as the shortest
// chunk length makes of the capacity - at least what the state-a-lane form may ask for
static inline uint64_t hml_cchunk_chunks(int mode, const hml_wl_geometry& g, uint64_t cap) {
    if (mode == HML_RTK_COMPAT) return HML_COMPAT_MAX_CHUNKS;
    const uint64_t n = (cap + g.min_L - 1) / g.min_L + 64;
    const uint64_t most = n < (uint64_t)HML_WL_MAX_CHUNKS ? n : (uint64_t)HML_WL_MAX_CHUNKS;
    return most > (uint64_t)HML_COMPAT_MAX_CHUNKS ? most : (uint64_t)HML_COMPAT_MAX_CHUNKS;
}
struct hml_cchunk_layout { hml_compat_chunks ch; uint64_t tot_bytes, bytes; };   // (tot_bytes: what the allocation clears)
static inline hml_cchunk_layout hml_layout_cchunk(void* base, int mode, const hml_wl_geometry& g, uint64_t cap, int K) {
    const uint64_t n = hml_cchunk_chunks(mode, g, cap);
    const uint64_t tot_words = mode == HML_RTK_COMPAT ? HML_COMPAT_TOT_WORDS : HML_WL_TOT_WORDS;
    hml_carver cv(base);
    hml_cchunk_layout l;
    l.ch.entry = cv.take<float>(n * K);
    l.ch.exitv = cv.take<float>(n * K);
    l.ch.nfb = cv.take<uint32_t>(n);
    l.ch.in_state = cv.take<int32_t>(n);
    l.ch.out_state = cv.take<int32_t>(n);
    l.ch.bad = cv.take<uint32_t>(n);
    l.ch.tot = cv.take<unsigned long long>(tot_words);
    l.ch.W = 0u;
    l.tot_bytes = tot_words * sizeof(unsigned long long);
    l.bytes = cv.bytes();
    return l;
}

// floats of one chunk-transposed [b][s] array of the chunk-a-lane path: L K cstride with cstride = the chunks rounded up to 64 - at
// most K (B + 64 L), L the longest chunk hml_k_wl_prepare can choose for this capacity (B <= cap)
static inline uint64_t hml_wl_plane_floats(const hml_wl_geometry& g, uint64_t cap, int K) {
    uint64_t Lmax = g.min_L > (1u << HML_WL_MIN_LSHIFT) ? g.min_L : (1u << HML_WL_MIN_LSHIFT);
    while ((cap + Lmax - 1) / Lmax > (uint64_t)g.max_chunks) Lmax *= 2;
    return (cap + 1 + 64 * Lmax) * K;
}

// ---- d_clists: the lists by state of the reference-compatible mode's count pass (hml_k_compat.h: "the count pass by STATE")
#define HML_COMPAT_PART_TILE 4096
struct hml_compat_lists {
    uint32_t* tile_count;   // [tiles][K] blocks of state s in the tile, then their exclusive prefix over the tiles
    uint32_t* state_off;    // [2 (K + 1)] first list position of state s (a multiple of four), then from K + 1 on the length of its list
    unsigned long long* offdiag;   // [K * K] transitions between different states
    // per list position, one array per quantity (round 5: each of the four wavefronts of the walk reads only what its chain adds -
    // sixteen entries are one 64-byte run per lane and array where they were sixteen 16-byte structures):
    float* sx;              // the block's Sx
    float* sq;              // the block's Sxx
    uint32_t* n;            // its size (below 2^31: the host takes the walk in block order for longer traces) and, in bit 31, whether
                            // the block before it has the same state (prev_0 = 0, ForwardBackward.hpp:172)
    // (every state's list starts at a multiple of four entries and the arrays are 16-byte aligned: four entries are one load;
    // the arrays hold B + 4 K entries)
};
static inline uint64_t hml_compat_tiles(uint64_t cap) { return (cap + HML_COMPAT_PART_TILE - 1) / HML_COMPAT_PART_TILE; }
struct hml_clists_layout { hml_compat_lists pl; uint64_t bytes; };
static inline hml_clists_layout hml_layout_clists(void* base, uint64_t cap, int K) {
    // entries of one list array: the blocks and up to three entries of padding per state, rounded to whole 16-byte groups
    const uint64_t entries = (cap + 4u * (uint64_t)HML_CAP_K + 3u) & ~(uint64_t)3u;
    hml_carver cv(base);
    hml_clists_layout l;
    l.pl.sx = cv.take<float>(entries, 16);
    l.pl.sq = cv.take<float>(entries, 16);
    l.pl.n = cv.take<uint32_t>(entries, 16);
    l.pl.offdiag = cv.take<unsigned long long>((uint64_t)HML_CAP_K * HML_CAP_K);
    l.pl.tile_count = cv.take<uint32_t>(hml_compat_tiles(cap) * K);
    l.pl.state_off = cv.take<uint32_t>(2 * (HML_CAP_K + 1));
    cv.slack(64);
    l.bytes = cv.bytes();
    return l;
}

// ---- d_wA: the transition matrix padded to 64 x 64 (hml_k_wl_prepare) and, behind it, the table of rescale factors (hml_k_wl_gtable)
#define HML_WL_PITCH 64   // floats between the rows of the padded transition matrix
#define HML_WL_GTAB 2048  // block sizes the table holds, per state
struct hml_wa_layout { float* A; float* gtab; uint64_t bytes; };
static inline hml_wa_layout hml_layout_wa(void* base) {
    hml_carver cv(base);
    hml_wa_layout l;
    l.A = cv.take<float>((uint64_t)HML_WL_PITCH * HML_WL_PITCH, 16);   // (read four floats at a time)
    l.gtab = cv.take<float>((uint64_t)HML_CAP_K * HML_WL_GTAB);
    l.bytes = cv.bytes();
    return l;
}

// ---- d_wave_total: per tile of the split many-chain block kernels (hml_k_blocks_split_many.h; `tiles`: those of one batch, the
// most there can be) the starts per wavefront and, behind them, the starts before the tile and the last start before it
#define HML_FUSED_WAVES 8   // wavefronts per workgroup of the block kernels
struct hml_wave_total_layout { uint32_t *wave_total, *tile_before, *tile_prev; uint64_t bytes; };
static inline hml_wave_total_layout hml_layout_wave_total(void* base, uint64_t tiles) {
    hml_carver cv(base);
    hml_wave_total_layout l;
    l.wave_total = cv.take<uint32_t>((tiles + 1) * HML_FUSED_WAVES);
    l.tile_before = cv.take<uint32_t>(tiles + 1);
    l.tile_prev = cv.take<uint32_t>(tiles + 1);
    l.bytes = cv.bytes();
    return l;
}

#endif

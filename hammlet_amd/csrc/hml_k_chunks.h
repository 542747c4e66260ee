// The repair scheme of the chunked recursions of exact inference (hml_infer.hip): the Viterbi decode
// (hml_k_viterbi.h), the two directions of the smoothing (hml_k_posterior.h) and the E-steps of many members (hml_k_em_many.h).
//
// A recursion over the blocks is one chain of dependent steps on a vector of K words.  It is cut into chunks, a chunk a lane, and
// a CHAIN INDEX x counts the chunks in the order of the recursion, so that the predecessor of x is x - 1.  The first run of
// chunk x starts some blocks early from a fixed vector and records entry[x], the vector it enters its own blocks with, and
// exit[x]; everything a chunk stores is a function of its entry vector alone.  Then, here:
//   verify    x matches iff entry[x] == exit[x - 1] in all K words, bit for bit.  When every chunk matches, induction from chunk 0
//             (whose first run is exact) makes every stored row the sequential recursion's.  The stale chunks are counted and
//             the HEADS of their runs - stale chunks whose predecessor matches - are listed;
//   rounds    a lane per head walks its run of stale chunks (hml_chunk_rerun_walk); all chunks are verified again;
//   finish    what the rounds leave is walked by one wavefront in increasing order (hml_chunk_finish_walk).
// The host's loop around them is repair_rounds (hml_infer.hip).  Two things vary: the stored word T (long long: the decode's
// fixed-point scores; double: the smoothing's probabilities) and run(x, from), which runs chunk x again from the vector at `from`
// - then its entry - and stores entry[x], exit[x] and the chunk's rows.  A chunk's first run never goes through it.
//
// The path sampler (hml_k_sample.h) is NOT an instance: its entry is one byte per (draw, chunk) pair, its rerun does not walk on
// and its finish is a lane per draw - a different and much simpler scheme, which has its own few lines.
//
// hml_chunk_same and hml_chunk_rerun_walk are plain C++ and compile for the host (tests/fixtures/chunk_walk_main.cpp walks
// a toy recursion with them); the verify body and the finishing walk use atomics and wavefront votes and are the device's alone.
#ifndef HML_K_CHUNKS_H
#define HML_K_CHUNKS_H

#include "hml_common.h"

HML_HD uint64_t hml_chunk_word(long long v) { return (uint64_t)v; }
HML_HD uint64_t hml_chunk_word(double v) { return hml_d2u(v); }   // (never ==: -0.0 against 0.0 and NaN payloads are differences)

// all K elements equal as 64-bit words.  They are read as T - doubles as doubles - and not through a pointer to words: the
// lane that compares may be the one that has just stored them
template <typename T>
HML_HD bool hml_chunk_same(const T* p, const T* q, int K) {
    bool eq = true;
    for (int j = 0; j < K; ++j) eq = eq && hml_chunk_word(p[j]) == hml_chunk_word(q[j]);
    return eq;
}

// A repair round, one lane's part: the walk from x, the head of a run of stale chunks (never chunk 0).  The head's predecessor
// matches, so nothing writes that exit vector in this round: the lane runs the head again from it, exactly, and walks on - a
// chunk whose entry equals the exit vector its predecessor has NOW stands as stored; any other runs again from that vector.
// The walk ends where a chunk that matched before still matches (nothing behind it has changed), and before it would rewrite a
// matching chunk whose successor is stale: that successor is another lane's head and reads this exit vector - no lane may
// rewrite an exit vector that another lane's head reads.  What such a stop leaves behind, the next verification finds.
// `match` is the last verification's and is only read here.
template <typename T, class Run>
HML_HD void hml_chunk_rerun_walk(Run run, const T* entry, const T* exitv, int K, uint32_t n_chunks, uint32_t x, const uint8_t* match) {
    for (;;) {
        run(x, exitv + (uint64_t)(x - 1u) * K);
        for (;;) {
            const uint32_t nx = x + 1u;
            if (nx >= n_chunks) return;
            const bool listed = match[nx] == 0;
            if (hml_chunk_same(entry + (uint64_t)nx * K, exitv + (uint64_t)x * K, K)) {
                if (!listed) return;   // it matched before and still does
                x = nx;                // stale before, right as stored now: on to its successor
                continue;
            }
            if (!listed && nx + 1u < n_chunks && match[nx + 1u] == 0) return;   // nx is the predecessor another lane reads
            x = nx;
            break;
        }
    }
}

#if defined(__HIPCC__)
// The grid-stride body of a verification: match[x] = (entry[x] == exit[x - 1]); the chunks that do not match are counted, the
// heads of their runs listed (in no order)
template <typename T>
__device__ __forceinline__ void hml_chunk_verify(const T* __restrict__ entry, const T* __restrict__ exitv, int K, uint32_t n_chunks, uint8_t* __restrict__ match,
                                                 uint32_t* __restrict__ heads, uint32_t* __restrict__ n_stale, uint32_t* __restrict__ n_heads) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t x = blockIdx.x * blockDim.x + threadIdx.x; x < n_chunks; x += stride) {
        const bool eq = x == 0u || hml_chunk_same(entry + (uint64_t)x * K, exitv + (uint64_t)(x - 1u) * K, K);
        match[x] = eq ? 1 : 0;
        if (!eq) {
            atomicAdd(n_stale, 1u);
            if (x == 1u || hml_chunk_same(entry + (uint64_t)(x - 1u) * K, exitv + (uint64_t)(x - 2u) * K, K)) heads[atomicAdd(n_heads, 1u)] = x;
        }
    }
}

// ... as a kernel of one pass, for the decode's words and the smoothing's
template <typename T>
HML_KERNEL __launch_bounds__(256) void hml_k_chunk_verify(const T* __restrict__ entry, const T* __restrict__ exitv, int K, uint32_t n_chunks, uint8_t* __restrict__ match,
                                                          uint32_t* __restrict__ heads, uint32_t* __restrict__ n_stale, uint32_t* __restrict__ n_heads) {
    hml_chunk_verify(entry, exitv, K, n_chunks, match, heads, n_stale, n_heads);
}

// What the rounds left: one wavefront (all 64 lanes call) walks the chain in increasing order - 64 match bytes at a time while
// nothing is stale - and its first lane runs every chunk that does not match its predecessor's exit vector as it stands then.
// The chunks it ran are ADDED to *walked: the smoothing's two directions share the word; the decode zeroes its words before
// the pass, so there it is the count itself.
template <typename T, class Run>
__device__ __forceinline__ void hml_chunk_finish_walk(Run run, const T* entry, const T* exitv, int K, uint32_t n_chunks, const uint8_t* __restrict__ match,
                                                      unsigned long long* __restrict__ walked) {
    const int lane = threadIdx.x;
    unsigned long long n_walked = 0ull;
    bool dirty = false;   // the predecessor was just run again: its exit vector is new
    for (uint64_t base = 1u; base < n_chunks; base += 64u) {
        const uint64_t mine = base + (uint32_t)lane;
        const bool stale = mine < n_chunks && match[mine] == 0;
        const unsigned long long mask = __ballot(stale);
        if (mask == 0ull && !dirty) continue;
        for (uint32_t k = 0; k < 64u && base + k < n_chunks; ++k) {
            const uint32_t x = (uint32_t)(base + k);
            int need = (int)((mask >> k) & 1ull);
            if (dirty) {
                if (lane == 0) need = hml_chunk_same(entry + (uint64_t)x * K, exitv + (uint64_t)(x - 1u) * K, K) ? 0 : 1;
                need = __shfl(need, 0);
            }
            if (need) {
                if (lane == 0) {
                    run(x, exitv + (uint64_t)(x - 1u) * K);
                    __threadfence();
                }
                ++n_walked;
            }
            dirty = need != 0;
            if (!dirty && (mask >> k) >> 1 == 0ull) break;   // nothing stale in the rest of these 64
        }
    }
    if (lane == 0) *walked += n_walked;
}
#endif

#endif

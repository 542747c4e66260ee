// Path sampling on the device (hml_posterior_sample, include/hml.h): independent draws of whole state paths from
// p(q | y, theta) over the current blocks under the current parameters.  hml_sample_ref.h states the definition and restates
// it for one host thread; DESIGN.md 3c, "Sampled paths".
//
// A draw is one chain of B dependent categorical draws, from the last block down; the draws of a call are independent.  The
// chain is cut as the decode and the smoothing are cut (hml_k_viterbi.h, hml_k_posterior.h), on a single integer word:
//   chunks    L blocks a chunk, counted from the LAST block: chunk k owns blocks [hi - L + 1, hi], hi = B - 1 - k L.  A lane is
//             one (draw, chunk) pair; a workgroup is 256 draws of one chunk, so its lanes read the same alpha row together;
//   first run chunk k starts at block hi + W with a guessed state - the smallest arg-max of alpha there - or, where that reaches
//             block B - 1, with the true first draw.  It walks down with the draw's own uniforms, which are addressed by
//             (draw, block) and not consumed in order, records entry[k] - the state it arrives with at block hi + 1 - and
//             exit[k], the state of its lowest block, and stores the states of its own blocks;
//   verify    k matches iff entry[k] == exit[k - 1]: everything a chunk stores is a function of its entry state alone, and
//             chunk 0 is exact - the induction of hml_k_viterbi.h.  A draw's chunk 0 compares with nothing;
//   repair    the heads of the stale runs (stale, predecessor not stale) run again from exit[k - 1] in parallel rounds; what
//             the rounds leave, a lane per draw walks in order.
// Paths are block-major with the draw fastest, so that a wavefront stores 64 consecutive bytes per block.  Everything derived
// from the paths is an integer sum, whose order is free.  W, L and the number of rounds decide which lane computes what, never
// a word of the result.
#ifndef HML_K_SAMPLE_H
#define HML_K_SAMPLE_H

#include "hml_k_pairs.h"   // (hml_pk_block_of; it brings hml_k_posterior.h)
#include "hml_sample_ref.h"

#define HML_SAMP_DEFAULT_L 256u   // (the draws supply the lanes: a longer chunk only walks less of its warm-up)
#define HML_SAMP_DEFAULT_W 256u   // ("Sampled paths")
#define HML_SAMP_LANES 256u       // draws of a workgroup

struct hml_samp_args {
    const double* alpha;         // [B][K]
    const double* A;             // [K][K]; the kernels keep its transpose in LDS
    const uint8_t* guess;        // [B]: the smallest arg-max of alpha_b
    int K;
    uint32_t B, L, W, n_chunks;
    uint32_t G;                  // draws of this group
    uint64_t first, seed;        // the group's first draw; the seed
    uint8_t* path;               // [B][G]
    uint8_t *entry, *exitv;      // [n_chunks][G]
    uint32_t* deg;               // [n_chunks][G]: degenerate blocks among a chunk's own, for the draw
};

// the transpose of A into LDS, rows padded by one double: sAT[q (K + 1) + i] = A[i][q]; every lane of the workgroup calls
__device__ __forceinline__ void hml_samp_stage(const hml_samp_args& a, double* sAT) {
    const int K = a.K;
    for (int x = threadIdx.x; x < K * K; x += blockDim.x) sAT[(x % K) * (K + 1) + x / K] = a.A[x];
    __syncthreads();
}

// a lane per block: the smallest arg-max of alpha_b
HML_KERNEL __launch_bounds__(256) void hml_k_samp_guess(const double* __restrict__ alpha, int K, uint32_t B, uint8_t* __restrict__ guess) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t b = blockIdx.x * blockDim.x + threadIdx.x; b < B; b += stride) {
        const double* const al = alpha + (uint64_t)b * K;
        int best = 0;
        for (int i = 1; i < K; ++i)
            if (al[i] > al[best]) best = i;
        guess[b] = (uint8_t)best;
    }
}

// hml_sample_ref_step: q_b from alpha_b and the successor's column of A (at == nullptr: the last block).  The weights are
// formed twice - for their sum, then for the search - by the same multiplication.
template <int KM>
__device__ __forceinline__ int hml_samp_step(int K, const double* __restrict__ al, const double* at, double u, uint32_t& n_deg) {
    constexpr int UF = KM <= 16 ? KM : 1;
    double S = 0.0;
#pragma unroll UF
    for (int i = 0; i < KM; ++i)
        if (i < K) S = S + (at ? al[i] * at[i] : al[i]);
    if (hml_sample_bad(S)) {
        ++n_deg;
        at = nullptr;
        S = 0.0;
#pragma unroll UF
        for (int i = 0; i < KM; ++i)
            if (i < K) S = S + al[i];
        if (hml_sample_bad(S)) return 0;
    }
    const double t = u * S;
    double c = 0.0;
    int found = -1, last = 0;
#pragma unroll UF
    for (int i = 0; i < KM; ++i)
        if (i < K) {
            const double w = at ? al[i] * at[i] : al[i];
            c = c + w;
            if (found < 0 && t < c) found = i;
            if (w > 0.0) last = i;
        }
    return found >= 0 ? found : last;
}

// the uniform of draw r at block b; a walk downwards meets the two blocks of a Philox word group one after the other
struct hml_samp_words { uint32_t index; hml_u32x4 o; };
__device__ __forceinline__ double hml_samp_uniform(hml_samp_words& w, uint64_t seed, uint64_t r, uint32_t b) {
    if (w.index != b >> 1) { w.index = b >> 1; w.o = hml_sample_words(seed, r, b >> 1); }
    return hml_sample_uniform_of(w.o, b);
}

// Chunk k of draw g by one lane.  from < 0: from the guess W blocks above (from the true first draw where that reaches block
// B - 1); else from that state as q_{hi + 1}, which is then the chunk's entry (k > 0).
template <int KM>
__device__ __forceinline__ void hml_samp_run_chunk(const hml_samp_args& a, const double* sAT, uint32_t k, uint32_t g, int from) {
    const int K = a.K;
    const int64_t B = a.B, G = a.G;
    const uint64_t r = a.first + g;
    const int64_t hi = B - 1 - (int64_t)k * a.L, lo = hi + 1 > (int64_t)a.L ? hi + 1 - (int64_t)a.L : 0;
    const uint64_t pair = (uint64_t)k * a.G + g;
    uint32_t n_deg = 0, scratch = 0;
    hml_samp_words words;
    words.index = 0xffffffffu;   // (no block has it)
    int q;
    int64_t b;   // the next block to draw
    if (from >= 0) {
        q = from;
        b = hi;
    } else if (hi + (int64_t)a.W >= B - 1) {
        q = hml_samp_step<KM>(K, a.alpha + (uint64_t)(B - 1) * K, nullptr, hml_samp_uniform(words, a.seed, r, (uint32_t)(B - 1)), k == 0u ? n_deg : scratch);
        if (k == 0u) a.path[(uint64_t)(B - 1) * G + g] = (uint8_t)q;
        b = B - 2;
    } else {
        q = a.guess[hi + a.W];
        b = hi + (int64_t)a.W - 1;
    }
    for (; b >= lo; --b) {
        const bool own = b <= hi;
        if (b == hi) a.entry[pair] = (uint8_t)q;   // (k > 0: chunk 0's highest block is B - 1, drawn above)
        q = hml_samp_step<KM>(K, a.alpha + (uint64_t)b * K, sAT + q * (K + 1), hml_samp_uniform(words, a.seed, r, (uint32_t)b), own ? n_deg : scratch);
        if (own) a.path[(uint64_t)b * G + g] = (uint8_t)q;
    }
    a.exitv[pair] = (uint8_t)q;
    a.deg[pair] = n_deg;
}

// first run: grid (chunk, draws / 256).  Dynamic LDS: K (K + 1) doubles, here and in the two kernels below
template <int KM>
HML_KERNEL __launch_bounds__(HML_SAMP_LANES) void hml_k_samp_first(const hml_samp_args a) {
    extern __shared__ double hml_samp_lds[];
    hml_samp_stage(a, hml_samp_lds);
    const uint32_t g = blockIdx.y * HML_SAMP_LANES + threadIdx.x;
    if (g >= a.G) return;
    hml_samp_run_chunk<KM>(a, hml_samp_lds, blockIdx.x, g, -1);
}

// a lane per (draw, chunk) pair, chunk 0 left out: stale pairs are counted, the heads of their runs counted and listed
HML_KERNEL __launch_bounds__(256) void hml_k_samp_verify(const uint8_t* __restrict__ entry, const uint8_t* __restrict__ exitv, uint32_t G, uint64_t n_pairs,
                                                         uint32_t* __restrict__ list, uint32_t* __restrict__ n_stale, uint32_t* __restrict__ n_heads) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t p = (uint64_t)G + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n_pairs; p += stride) {
        if (entry[p] == exitv[p - G]) continue;
        atomicAdd(n_stale, 1u);
        if (p >= 2ull * G && entry[p - G] != exitv[p - 2ull * G]) continue;   // its predecessor is stale too
        list[atomicAdd(n_heads, 1u)] = (uint32_t)p;
    }
}

// a repair round: a lane per head, from its predecessor's exit (which no lane of this launch writes)
template <int KM>
HML_KERNEL __launch_bounds__(64) void hml_k_samp_rerun(const hml_samp_args a, const uint32_t* __restrict__ list, uint32_t n_heads) {
    extern __shared__ double hml_samp_lds[];
    hml_samp_stage(a, hml_samp_lds);
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n_heads) return;
    const uint32_t p = list[i], k = p / a.G, g = p % a.G;
    hml_samp_run_chunk<KM>(a, hml_samp_lds, k, g, a.exitv[p - a.G]);
}

// what the rounds left: a lane per draw walks its chunks in order and runs what does not match
template <int KM>
HML_KERNEL __launch_bounds__(64) void hml_k_samp_finish(const hml_samp_args a, unsigned long long* __restrict__ walked) {
    extern __shared__ double hml_samp_lds[];
    hml_samp_stage(a, hml_samp_lds);
    const uint32_t g = blockIdx.x * 64u + threadIdx.x;
    if (g >= a.G) return;
    unsigned long long n = 0ull;
    for (uint32_t k = 1u; k < a.n_chunks; ++k) {
        const uint8_t e = a.exitv[(uint64_t)(k - 1u) * a.G + g];
        if (a.entry[(uint64_t)k * a.G + g] == e) continue;
        hml_samp_run_chunk<KM>(a, hml_samp_lds, k, g, e);
        ++n;
    }
    if (n) atomicAdd(walked, n);
}

// the sum of deg[n_pairs] into *total
HML_KERNEL __launch_bounds__(256) void hml_k_samp_deg_sum(const uint32_t* __restrict__ deg, uint64_t n_pairs, unsigned long long* __restrict__ total) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    unsigned long long s = 0ull;
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n_pairs; p += stride) s += deg[p];
    if (s) atomicAdd(total, s);
}

// per draw, from the finished paths: changes (segments - 1) and the score in the decode's tables; grid and lanes as the first
// run's.  emit == nullptr: the changes alone
HML_KERNEL __launch_bounds__(HML_SAMP_LANES) void hml_k_samp_draw_stats(const hml_samp_args a, const long long* __restrict__ emit, const long long* __restrict__ trans,
                                                                        const long long* __restrict__ init, unsigned long long* __restrict__ changes,
                                                                        unsigned long long* __restrict__ score) {
    const uint32_t g = blockIdx.y * HML_SAMP_LANES + threadIdx.x;
    if (g >= a.G) return;
    const int K = a.K;
    const int64_t B = a.B, G = a.G;
    const int64_t hi = B - 1 - (int64_t)blockIdx.x * a.L, lo = hi + 1 > (int64_t)a.L ? hi + 1 - (int64_t)a.L : 0;
    unsigned long long n = 0ull, s = 0ull;
    int prev = lo > 0 ? a.path[(uint64_t)(lo - 1) * G + g] : -1;
    for (int64_t b = lo; b <= hi; ++b) {
        const int q = a.path[(uint64_t)b * G + g];
        if (prev >= 0 && q != prev) ++n;
        if (emit) s += (unsigned long long)emit[(uint64_t)b * K + q] + (unsigned long long)(prev >= 0 ? trans[prev * K + q] : init[q]);
        prev = q;
    }
    if (n) atomicAdd(changes + g, n);
    if (emit) atomicAdd(score + g, s);
}

// per block, over the draws of the group: a wavefront per block adds to change_count[b] and, if given, state_count[b][K]
HML_KERNEL __launch_bounds__(64) void hml_k_samp_block_counts(const uint8_t* __restrict__ path, int K, uint32_t B, uint32_t G, uint32_t* __restrict__ change_count,
                                                              uint32_t* __restrict__ state_count) {
    __shared__ uint32_t cnt[HML_CAP_K + 1];
    const int lane = threadIdx.x;
    for (uint32_t b = blockIdx.x; b < B; b += gridDim.x) {
        cnt[lane] = 0u;
        if (lane == 0) cnt[HML_CAP_K] = 0u;
        __syncthreads();
        const uint8_t* const row = path + (uint64_t)b * G;
        uint32_t n = 0u;
        for (uint32_t g = lane; g < G; g += 64u) {
            const uint8_t q = row[g];
            if (state_count) atomicAdd(&cnt[q], 1u);
            if (b > 0u && q != (row - G)[g]) ++n;
        }
        if (n) atomicAdd(&cnt[HML_CAP_K], n);
        __syncthreads();
        if (state_count && lane < K) state_count[(uint64_t)b * K + lane] += cnt[lane];
        if (lane == 0) change_count[b] += cnt[HML_CAP_K];
        __syncthreads();
    }
}

// path[B][G] -> out[G][B], 64 x 64 tiles through LDS
HML_KERNEL __launch_bounds__(256) void hml_k_samp_transpose(const uint8_t* __restrict__ path, uint32_t B, uint32_t G, uint8_t* __restrict__ out) {
    __shared__ uint8_t tile[64][65];
    const uint32_t tx = threadIdx.x & 63u, ty = threadIdx.x >> 6;
    const uint64_t b0 = (uint64_t)blockIdx.x * 64u, g0 = (uint64_t)blockIdx.y * 64u;
    for (uint32_t i = ty; i < 64u; i += 4u)
        if (b0 + i < B && g0 + tx < G) tile[i][tx] = path[(b0 + i) * G + g0 + tx];
    __syncthreads();
    for (uint32_t i = ty; i < 64u; i += 4u)
        if (g0 + i < G && b0 + tx < B) out[(g0 + i) * B + b0 + tx] = tile[tx][i];
}

// the region counts: a lane per (draw, region), grid (draws / 256, regions); every count an integer addition
struct hml_samp_regions_out {
    uint32_t *hist, *whole_state;            // [n][H + 1], [n][K]
    unsigned long long *breaks_sum, *breaks_sq;   // [n]
};
HML_KERNEL __launch_bounds__(256) void hml_k_samp_regions(const uint8_t* __restrict__ path, const uint32_t* __restrict__ starts, int K, uint32_t B, uint32_t G,
                                                          const uint32_t* __restrict__ start, const uint32_t* __restrict__ end, uint64_t n, uint32_t H,
                                                          hml_samp_regions_out o) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g >= G) return;
    for (uint64_t i = blockIdx.y; i < n; i += gridDim.y) {
        const uint32_t ba = hml_pk_block_of(starts, B, start[i]), be = hml_pk_block_of(starts, B, end[i] - 1u);
        int prev = path[(uint64_t)ba * G + g];
        const int qa = prev;
        unsigned long long m = 0ull;
        for (uint64_t b = (uint64_t)ba + 1u; b <= be; ++b) {
            const int q = path[b * G + g];
            m += q != prev;
            prev = q;
        }
        atomicAdd(o.hist + i * (H + 1u) + (m < H ? (uint32_t)m : H), 1u);
        if (m == 0ull) atomicAdd(o.whole_state + i * K + qa, 1u);
        else {
            atomicAdd(o.breaks_sum + i, m);
            atomicAdd(o.breaks_sq + i, m * m);
        }
    }
}

#endif

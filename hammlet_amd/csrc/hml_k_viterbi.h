// Viterbi decode on the device (hml_viterbi, include/hml.h): the jointly most probable state path over the current blocks
// under the current parameters, as a FIXED-POINT max-plus recursion - every score an int64 in units of 2^-20 nat
// (hml_viterbi_ref.h states the definition and restates it for one host thread; DESIGN.md 3c, "Viterbi decode").
//
// The recursion over B blocks is one chain of dependent steps.  It is cut into chunks of L blocks, a chunk a lane:
//   forward   chunk c starts W blocks early from the zero vector (chunk 0, and every chunk whose warm-up reaches block 0, from
//             `init`: exact), records entry[c] - its normalised vector at block c L - 1 - and exit[c], and stores the
//             back-pointers psi of its own blocks;
//   verify, repair   the scheme of hml_k_chunks.h on the K integer words: two runs that have coalesced hold the same normalised
//             vector exactly; the rounds from the heads of the stale runs, then one wavefront's walk;
//   backtrack per chunk the map [K] -> [K] from its end state to the end state of its predecessor, the maps composed over
//             groups of chunks, one lane down the groups, then the chunks of a group, then every chunk walks its rows.
// W, L and the number of rounds decide which lane computes what, never a word of the result.
#ifndef HML_K_VITERBI_H
#define HML_K_VITERBI_H

#include "hml_k_blocks.h"
#include "hml_k_chunks.h"
#include "hml_k_forward.h"
#include "hml_math.h"
#include "hml_state.h"

#define HML_VIT_DEFAULT_L 64u
#define HML_VIT_DEFAULT_W 64u

// fx of hml_viterbi_ref.h (the product is exact: |x| <= 2^38)
__device__ __forceinline__ long long hml_vit_fx(double x) {
    const double lim = 274877906944.0;   // 2^38
    if (!(x == x)) x = -lim;
    x = x < -lim ? -lim : x;
    x = x > lim ? lim : x;
    return __double2ll_rn(x * 1048576.0);
}

// what the emission terms need, derived from mu, var and A by hml_derive's formulas (not read from the model's logN / logA: a
// reference-compatible context keeps glibc's values there)
struct hml_vit_par {
    int32_t K, D, P, self;
    uint32_t T, B;
    float mu[HML_CAP_K], var[HML_CAP_K];
    double rvar2[HML_CAP_K];
    float logNs[HML_CAP_K], logA[HML_CAP_K];
    uint8_t map[HML_CAP_K][HML_MAX_D];
};

// the parameters, by the first K lanes of a workgroup
__device__ __forceinline__ void hml_vit_par_fill(const hml_model* __restrict__ mdl, hml_vit_par* __restrict__ par, int tid) {
    const int K = mdl->K, D = mdl->D, P = mdl->P;
    if (tid == 0) { par->K = K; par->D = D; par->P = P; par->self = mdl->self_trans != 0; par->T = mdl->T; par->B = mdl->B; }
    if (tid < P) {
        const float v = mdl->var[tid];
        par->mu[tid] = mdl->mu[tid]; par->var[tid] = v;
        par->rvar2[tid] = 1.0 / (2.0 * (double)v);
    }
    if (tid < K) {
        float r = 0.0f;
        for (int d = 0; d < D; ++d) {
            const int pp = mdl->map[tid][d];
            const float m = mdl->mu[pp], v = mdl->var[pp], sd = HML_SQRTF(v);
            r += hml_logf(sd) + m * m / (2 * v);
        }
        par->logNs[tid] = r;
        par->logA[tid] = hml_logf(mdl->A[tid * K + tid]);
        for (int d = 0; d < HML_MAX_D; ++d) par->map[tid][d] = mdl->map[tid][d];
    }
}

// one workgroup of 256: the parameters, init[K] and trans[K][K]
HML_KERNEL __launch_bounds__(256) void hml_k_vit_tables(const hml_model* __restrict__ mdl, hml_vit_par* __restrict__ par,
                                                        long long* __restrict__ trans, long long* __restrict__ init) {
    const int tid = threadIdx.x, K = mdl->K;
    hml_vit_par_fill(mdl, par, tid);
    if (tid < K) init[tid] = hml_vit_fx((double)hml_logf(mdl->pi[tid]));
    for (int i = tid; i < K * K; i += 256) trans[i] = hml_vit_fx((double)hml_logf(mdl->A[i]));
}

// the statistics of block b, recomputed from the integral array(s)
struct hml_vit_block {
    float sx[HML_MAX_D], sq[HML_MAX_D], N;
};
__device__ __forceinline__ void hml_vit_block_load(const hml_vit_par* __restrict__ par, const float2* __restrict__ ia,
                                                   const uint32_t* __restrict__ starts, uint32_t b, hml_vit_block& blk) {
    const uint32_t st = starts[b], en = starts[b + 1];
    const int D = par->D;
    const uint64_t plane = (uint64_t)par->T + 1u;
#pragma unroll
    for (int d = 0; d < HML_MAX_D; ++d)
        if (d < D) hml_block_stats_one(ia + (uint64_t)d * plane, st, en, blk.sx[d], blk.sq[d]);
    blk.N = (float)(en - st);
}
// E_b(s) of hml_emit_compute / hml_k_emission_mv
__device__ __forceinline__ float hml_vit_emit_float(const hml_vit_par* __restrict__ par, const hml_vit_block& blk, int s) {
    const int D = par->D;
    float r = 0.0f;
#pragma unroll
    for (int d = 0; d < HML_MAX_D; ++d) {
        if (d < D) {
            const int pp = par->map[s][d];
            r += hml_inner_product(par->mu[pp], par->var[pp], par->rvar2[pp], blk.sx[d], blk.sq[d]);
        }
    }
    float e = r - blk.N * par->logNs[s];
    if (par->self) e += (blk.N - 1.0f) * par->logA[s];
    return e;
}
// emit[b][s]: the same, quantised
__device__ __forceinline__ long long hml_vit_emit(const hml_vit_par* __restrict__ par, const hml_vit_block& blk, int s) {
    return hml_vit_fx((double)hml_vit_emit_float(par, blk, s));
}

// probe: the whole table emit[B][K], a lane per block
HML_KERNEL __launch_bounds__(256) void hml_k_vit_emit_table(const hml_vit_par* __restrict__ par, const float2* __restrict__ ia,
                                                            const uint32_t* __restrict__ starts, long long* __restrict__ emit) {
    const uint32_t B = par->B;
    const int K = par->K;
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t b = blockIdx.x * blockDim.x + threadIdx.x; b < B; b += stride) {
        hml_vit_block blk;
        hml_vit_block_load(par, ia, starts, b, blk);
        for (int s = 0; s < K; ++s) emit[(uint64_t)b * K + s] = hml_vit_emit(par, blk, s);
    }
}

// what a run over a chunk reads and writes
struct hml_vit_args {
    const hml_vit_par* par;
    const long long *trans, *init;
    const float2* ia;
    const uint32_t* starts;
    uint32_t L, W, n_chunks;
    long long *entry, *exitv;    // [n_chunks][K]
    uint8_t* psi;                // [B][K]
};

// The recursion over blocks [first, end of chunk c) by one lane.  from == nullptr: from the zero vector (from `init` if
// first == 0); else from that normalised vector, which is then the chunk's entry.  KM: the states the vector is kept for -
// registers up to 16 (loops unrolled), a per-lane array beyond (KM = HML_CAP_K, loops kept).
// The tables come apart again as __restrict__ parameters: only so does the compiler know that the bytes stored to psi leave
// them alone, and keep their loads scalar.
template <int KM>
__device__ __forceinline__ void hml_vit_recursion(const hml_vit_par* __restrict__ par, const long long* __restrict__ trans, const long long* __restrict__ init,
                                                  const float2* __restrict__ ia, const uint32_t* __restrict__ starts, uint32_t L, uint32_t c, uint32_t first,
                                                  const long long* from, long long* entry, long long* exitv, uint8_t* psi) {
    constexpr int UF = KM <= 16 ? KM : 1;
    const int K = par->K;
    const uint32_t B = par->B;
    const uint64_t lo64 = (uint64_t)c * L, hi64 = lo64 + L < (uint64_t)B ? lo64 + L : (uint64_t)B;
    const uint32_t lo = (uint32_t)lo64, hi = (uint32_t)hi64;
    long long d[KM], nd[KM];
#pragma unroll UF
    for (int j = 0; j < KM; ++j)
        if (j < K) {
            d[j] = from ? from[j] : 0ll;
            if (from || lo == 0u) entry[(uint64_t)c * K + j] = d[j];
        }
    for (uint32_t b = first; b < hi; ++b) {
        hml_vit_block blk;
        hml_vit_block_load(par, ia, starts, b, blk);
        const bool own = b >= lo;
        long long top = (long long)0x8000000000000000ull;
#pragma unroll UF
        for (int j = 0; j < KM; ++j) {
            if (j < K) {
                long long best;
                int arg = 0;
                if (b == 0u) best = init[j];
                else {
                    best = d[0] + trans[j];
#pragma unroll UF
                    for (int i = 1; i < KM; ++i) {
                        if (i < K) {
                            const long long v = d[i] + trans[i * K + j];
                            if (v > best) { best = v; arg = i; }
                        }
                    }
                }
                const long long v = best + hml_vit_emit(par, blk, j);
                nd[j] = v;
                top = v > top ? v : top;
                if (own) psi[(uint64_t)b * K + j] = (uint8_t)arg;
            }
        }
        const bool is_entry = b + 1u == lo;
#pragma unroll UF
        for (int j = 0; j < KM; ++j)
            if (j < K) {
                d[j] = nd[j] - top;
                if (is_entry) entry[(uint64_t)c * K + j] = d[j];
            }
    }
#pragma unroll UF
    for (int j = 0; j < KM; ++j)
        if (j < K) exitv[(uint64_t)c * K + j] = d[j];
}
// ... of the pass `a` describes: what the kernels and the walks call
template <int KM>
__device__ __forceinline__ void hml_vit_run_chunk(const hml_vit_args& a, uint32_t c, uint32_t first, const long long* from) {
    hml_vit_recursion<KM>(a.par, a.trans, a.init, a.ia, a.starts, a.L, c, first, from, a.entry, a.exitv, a.psi);
}

// first pass: a lane per chunk, W blocks of warm-up
template <int KM>
HML_KERNEL __launch_bounds__(64) void hml_k_vit_forward(const hml_vit_args a) {
    const uint32_t c = blockIdx.x * 64u + threadIdx.x;
    if (c >= a.n_chunks) return;
    const uint64_t lo = (uint64_t)c * a.L;
    hml_vit_run_chunk<KM>(a, c, lo > a.W ? (uint32_t)(lo - a.W) : 0u, nullptr);
}

// a repair round: a lane per head (hml_chunk_rerun_walk)
template <int KM>
HML_KERNEL __launch_bounds__(64) void hml_k_vit_rerun(const hml_vit_args a, const uint32_t* __restrict__ heads, uint32_t n_heads, const uint8_t* __restrict__ match) {
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n_heads) return;
    auto run = [&](uint32_t x, const long long* from) { hml_vit_run_chunk<KM>(a, x, (uint32_t)((uint64_t)x * a.L), from); };
    hml_chunk_rerun_walk(run, a.entry, a.exitv, a.par->K, a.n_chunks, heads[i], match);
}

// what the rounds left: one wavefront (hml_chunk_finish_walk)
template <int KM>
HML_KERNEL __launch_bounds__(64) void hml_k_vit_finish(const hml_vit_args a, const uint8_t* __restrict__ match, unsigned long long* __restrict__ walked) {
    if (blockIdx.x != 0u || blockDim.x != 64u) return;
    auto run = [&](uint32_t x, const long long* from) { hml_vit_run_chunk<KM>(a, x, (uint32_t)((uint64_t)x * a.L), from); };
    hml_chunk_finish_walk(run, a.entry, a.exitv, a.par->K, a.n_chunks, match, walked);
}

// maps[c][j]: the state at the last block of chunk c - 1 when block (end of chunk c) is in state j  (chunk 0: unused)
HML_KERNEL __launch_bounds__(64) void hml_k_vit_chunk_maps(const uint8_t* __restrict__ psi, int K, uint32_t B, uint32_t L, uint32_t n_chunks,
                                                           uint8_t* __restrict__ maps) {
    const uint32_t c = blockIdx.x * 64u + threadIdx.x;
    if (c >= n_chunks) return;
    const uint64_t lo = (uint64_t)c * L, hi = lo + L < (uint64_t)B ? lo + L : (uint64_t)B;
    for (int j = 0; j < K; ++j) {
        uint32_t s = (uint32_t)j;
        for (uint64_t b = hi; b-- > lo;)
            if (b > 0u) s = psi[b * K + s];
        maps[(uint64_t)c * K + j] = (uint8_t)s;
    }
}

// the chunk maps of group u (S chunks) composed: gmaps[u][j] = the state at the end of the chunk before the group
HML_KERNEL __launch_bounds__(64) void hml_k_vit_group_maps(const uint8_t* __restrict__ maps, int K, uint32_t n_chunks, uint32_t S, uint32_t n_groups,
                                                           uint8_t* __restrict__ gmaps) {
    const uint32_t u = blockIdx.x * 64u + threadIdx.x;
    if (u >= n_groups) return;
    const uint64_t lo = (uint64_t)u * S, hi = lo + S < (uint64_t)n_chunks ? lo + S : (uint64_t)n_chunks;
    for (int j = 0; j < K; ++j) {
        uint32_t s = (uint32_t)j;
        for (uint64_t c = hi; c-- > lo;)
            if (c > 0u) s = maps[c * K + s];
        gmaps[(uint64_t)u * K + j] = (uint8_t)s;
    }
}

// one lane: the end state - the smallest j with exit[last chunk][j] == 0 - and from it the end state of every group
HML_KERNEL __launch_bounds__(64) void hml_k_vit_group_ends(const long long* __restrict__ exitv, const uint8_t* __restrict__ gmaps, int K,
                                                           uint32_t n_chunks, uint32_t n_groups, uint8_t* __restrict__ gend) {
    if (blockIdx.x != 0u || threadIdx.x != 0u) return;
    uint32_t s = 0;
    while (s + 1u < (uint32_t)K && exitv[(uint64_t)(n_chunks - 1u) * K + s] != 0ll) ++s;
    for (uint32_t u = n_groups; u-- > 0u;) {
        gend[u] = (uint8_t)s;
        s = gmaps[(uint64_t)u * K + s];
    }
}

// a lane per group: the end state of each of its chunks
HML_KERNEL __launch_bounds__(64) void hml_k_vit_chunk_ends(const uint8_t* __restrict__ maps, const uint8_t* __restrict__ gend, int K,
                                                           uint32_t n_chunks, uint32_t S, uint32_t n_groups, uint8_t* __restrict__ cend) {
    const uint32_t u = blockIdx.x * 64u + threadIdx.x;
    if (u >= n_groups) return;
    const uint64_t lo = (uint64_t)u * S, hi = lo + S < (uint64_t)n_chunks ? lo + S : (uint64_t)n_chunks;
    uint32_t s = gend[u];
    for (uint64_t c = hi; c-- > lo;) {
        cend[c] = (uint8_t)s;
        if (c > 0u) s = maps[c * K + s];
    }
}

// a lane per chunk: its rows from its end state
HML_KERNEL __launch_bounds__(64) void hml_k_vit_walk(const uint8_t* __restrict__ psi, const uint8_t* __restrict__ cend, int K, uint32_t B,
                                                     uint32_t L, uint32_t n_chunks, int16_t* __restrict__ q) {
    const uint32_t c = blockIdx.x * 64u + threadIdx.x;
    if (c >= n_chunks) return;
    const uint64_t lo = (uint64_t)c * L, hi = lo + L < (uint64_t)B ? lo + L : (uint64_t)B;
    uint32_t s = cend[c];
    for (uint64_t b = hi; b-- > lo;) {
        q[b] = (int16_t)s;
        if (b > 0u) s = psi[b * K + s];
    }
}

// the path's score: init, emit and trans along q, an order-free sum of 64-bit words (two's complement)
HML_KERNEL __launch_bounds__(256) void hml_k_vit_score(const hml_vit_par* __restrict__ par, const long long* __restrict__ trans,
                                                       const long long* __restrict__ init, const float2* __restrict__ ia,
                                                       const uint32_t* __restrict__ starts, const int16_t* __restrict__ q,
                                                       unsigned long long* __restrict__ score) {
    const uint32_t B = par->B;
    const int K = par->K;
    unsigned long long sum = 0ull;
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t b = blockIdx.x * blockDim.x + threadIdx.x; b < B; b += stride) {
        hml_vit_block blk;
        hml_vit_block_load(par, ia, starts, b, blk);
        const int s = q[b];
        sum += (unsigned long long)hml_vit_emit(par, blk, s);
        sum += (unsigned long long)(b == 0u ? init[s] : trans[(int)q[b - 1u] * K + s]);
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) sum += (unsigned long long)__shfl_xor((long long)sum, m);
    if ((threadIdx.x & 63u) == 0u) atomicAdd(score, sum);
}

#endif

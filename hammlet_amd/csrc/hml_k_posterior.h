// Smoothing on the device (hml_posterior, include/hml.h): the state posteriors gamma_b(j) = p(q_b = j | y, theta) over the
// current blocks under the current parameters, log p(y | theta) and the call per block - the sum-product sibling of the Viterbi
// decode.  hml_posterior_ref.h states the definition and restates it for one host thread; DESIGN.md 3c, "Smoothing".
//
// The float tables (E, m, e) are the sweep's; everything after them is IEEE double in a fixed order.  The forward and the
// backward recursion are each one chain of B dependent steps, cut exactly as the Viterbi decode is cut (hml_k_viterbi.h):
//   first run chunk x (a chain index, hml_k_chunks.h: forward x = chunk, backward x = n_chunks - 1 - chunk) starts W blocks
//             outside its blocks from the uniform vector (exact where that reaches block 0 - pi - or the last block), records
//             entry[x] and exit[x] and stores the rows (alpha_b and c_b, or beta_b) of its own blocks;
//   verify, repair   the scheme of hml_k_chunks.h on the K doubles, bit for bit: two runs of a normalised recursion that have
//             forgotten their start hold the same vector exactly;
//   combine   a lane per block: gamma_b, the called state and its posterior; l_b = m_b + log c_b was stored by the forward
//             run and is reduced by the fan-in-64 tree of the definition, a lane per value of the next level.
// W, L and the number of rounds decide which lane computes what, never a word of the result.
#ifndef HML_K_POSTERIOR_H
#define HML_K_POSTERIOR_H

#include "hml_k_viterbi.h"

#define HML_POST_DEFAULT_L 64u
#define HML_POST_DEFAULT_W 256u   // (measured: DESIGN.md 3c, "Smoothing", Cost)

__device__ __forceinline__ bool hml_post_bad(double x) { return !(x > 0.0 && x < hml_u2d(0x7ff0000000000000ull)); }

// one workgroup of 256: the parameters, and A[K][K] and pi[K] widened to double
HML_KERNEL __launch_bounds__(256) void hml_k_post_tables(const hml_model* __restrict__ mdl, hml_vit_par* __restrict__ par,
                                                         double* __restrict__ A, double* __restrict__ pi) {
    const int tid = threadIdx.x, K = mdl->K;
    hml_vit_par_fill(mdl, par, tid);
    if (tid < K) pi[tid] = (double)mdl->pi[tid];
    for (int i = tid; i < K * K; i += 256) A[i] = (double)mdl->A[i];
}

// what a run over a chunk reads and writes (one direction)
struct hml_post_args {
    const hml_vit_par* par;
    const double *A, *pi;        // global; the kernels keep a copy in LDS
    const float2* ia;
    const uint32_t* starts;
    uint32_t L, W, n_chunks;
    double *entry, *exitv;       // [n_chunks][K], by chain index
    double* rows;                // [B][K]: alpha or beta
    double *cval, *ell;          // [B]: c_b and l_b (forward only)
};

// A and pi into LDS (sA[K K], then sPi[K]); every lane of the workgroup calls
__device__ __forceinline__ void hml_post_stage(const hml_post_args& a, int K, double* sA) {
    for (int i = threadIdx.x; i < K * K; i += blockDim.x) sA[i] = a.A[i];
    for (int i = threadIdx.x; i < K; i += blockDim.x) sA[K * K + i] = a.pi[i];
    __syncthreads();
}

// m_b and e_b(j) of block b into e[KM]
template <int KM>
__device__ __forceinline__ float hml_post_terms(const hml_vit_par* __restrict__ par, const float2* __restrict__ ia, const uint32_t* __restrict__ starts,
                                                uint32_t b, float (&e)[KM]) {
    constexpr int UF = KM <= 16 ? KM : 1;
    const int K = par->K;
    hml_vit_block blk;
    hml_vit_block_load(par, ia, starts, b, blk);
    float top = -3.40282346638528859812e+38f;
#pragma unroll UF
    for (int j = 0; j < KM; ++j)
        if (j < K) {
            const float v = hml_vit_emit_float(par, blk, j);
            e[j] = v;
            top = (v < top) ? top : v;
        }
#pragma unroll UF
    for (int j = 0; j < KM; ++j)
        if (j < K) e[j] = hml_expf(e[j] - top);
    return top;
}

// probe: the whole tables e[B][K] and m[B], a lane per block
HML_KERNEL __launch_bounds__(256) void hml_k_post_term_table(const hml_vit_par* __restrict__ par, const float2* __restrict__ ia,
                                                             const uint32_t* __restrict__ starts, float* __restrict__ e_out, float* __restrict__ m_out) {
    const uint32_t B = par->B;
    const int K = par->K;
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t b = blockIdx.x * blockDim.x + threadIdx.x; b < B; b += stride) {
        float e[HML_CAP_K];
        const float top = hml_post_terms<HML_CAP_K>(par, ia, starts, b, e);
        if (m_out) m_out[b] = top;
        if (e_out)
            for (int j = 0; j < K; ++j) e_out[(uint64_t)b * K + j] = e[j];
    }
}

// The forward recursion over the blocks of chunk x by one lane.  from == nullptr: from the uniform vector W blocks early (from pi
// where that reaches block 0); else from that normalised vector, which is then the chunk's entry.  KM as in hml_vit_run_chunk.
template <int KM>
__device__ __forceinline__ void hml_post_forward_chunk(const hml_post_args& a, const double* sA, uint32_t x, const double* from) {
    constexpr int UF = KM <= 16 ? KM : 1;
    const hml_vit_par* const par = a.par;
    const int K = par->K;
    const uint32_t B = par->B;
    const double* const sPi = sA + K * K;
    const uint64_t lo64 = (uint64_t)x * a.L, hi64 = lo64 + a.L < (uint64_t)B ? lo64 + a.L : (uint64_t)B;
    const uint32_t lo = (uint32_t)lo64, hi = (uint32_t)hi64;
    const uint32_t first = from ? lo : (lo64 > a.W ? (uint32_t)(lo64 - a.W) : 0u);
    const double uni = 1.0 / (double)K;
    double d[KM], nd[KM];
    float e[KM];
#pragma unroll UF
    for (int j = 0; j < KM; ++j)
        if (j < K) {
            d[j] = from ? from[j] : uni;
            if (from || lo == 0u) a.entry[(uint64_t)x * K + j] = d[j];
        }
    for (uint32_t b = first; b < hi; ++b) {
        const float top = hml_post_terms<KM>(par, a.ia, a.starts, b, e);
        double c = 0.0;
#pragma unroll UF
        for (int j = 0; j < KM; ++j) {
            if (j < K) {
                double v;
                if (b == 0u) v = sPi[j] * (double)e[j];
                else {
                    double s = 0.0;
#pragma unroll UF
                    for (int i = 0; i < KM; ++i)
                        if (i < K) s = s + d[i] * sA[i * K + j];
                    v = (double)e[j] * s;
                }
                nd[j] = v;
                c = c + v;
            }
        }
        const bool bad = hml_post_bad(c);
        const bool own = b >= lo, is_entry = b + 1u == lo;
#pragma unroll UF
        for (int j = 0; j < KM; ++j)
            if (j < K) {
                const double v = bad ? uni : nd[j] / c;
                d[j] = v;
                if (own) a.rows[(uint64_t)b * K + j] = v;
                if (is_entry) a.entry[(uint64_t)x * K + j] = v;
            }
        if (own) {
            a.cval[b] = c;
            a.ell[b] = (double)top + hml_log(c);
        }
    }
#pragma unroll UF
    for (int j = 0; j < KM; ++j)
        if (j < K) a.exitv[(uint64_t)x * K + j] = d[j];
}

// The backward recursion over the blocks [lo, hi) of chunk n_chunks - 1 - x by one lane, downwards.  Its entry is beta_hi (for
// the last chunk nothing: beta_{B-1} is uniform by definition), its exit beta_lo.  from == nullptr: from the uniform vector at
// block hi + W (at block B - 1 where that reaches it: exact); else from that vector as beta_hi.
template <int KM>
__device__ __forceinline__ void hml_post_backward_chunk(const hml_post_args& a, const double* sA, uint32_t x, const double* from) {
    constexpr int UF = KM <= 16 ? KM : 1;
    const hml_vit_par* const par = a.par;
    const int K = par->K;
    const uint32_t B = par->B;
    const uint32_t ch = a.n_chunks - 1u - x;
    const uint64_t lo64 = (uint64_t)ch * a.L, hi64 = lo64 + a.L < (uint64_t)B ? lo64 + a.L : (uint64_t)B;
    const uint32_t lo = (uint32_t)lo64, hi = (uint32_t)hi64;
    uint32_t cur;   // d = beta_cur
    if (from) cur = hi;
    else cur = hi64 + a.W < (uint64_t)B - 1u ? (uint32_t)(hi64 + a.W) : B - 1u;
    const double uni = 1.0 / (double)K;
    double d[KM], v[KM];
    float e[KM];
    const bool at_start = cur == hi || hi == B;   // the entry is known now (the last chunk's: unused, the uniform vector)
#pragma unroll UF
    for (int j = 0; j < KM; ++j)
        if (j < K) {
            d[j] = from ? from[j] : uni;
            if (at_start) a.entry[(uint64_t)x * K + j] = d[j];
            if (cur < hi) a.rows[(uint64_t)cur * K + j] = d[j];   // (block B - 1 of the last chunk)
        }
    while (cur > lo) {
        (void)hml_post_terms<KM>(par, a.ia, a.starts, cur, e);
#pragma unroll UF
        for (int j = 0; j < KM; ++j)
            if (j < K) v[j] = (double)e[j] * d[j];
        double s = 0.0;
#pragma unroll UF
        for (int i = 0; i < KM; ++i) {
            if (i < K) {
                double t = 0.0;
#pragma unroll UF
                for (int j = 0; j < KM; ++j)
                    if (j < K) t = t + sA[i * K + j] * v[j];
                d[i] = t;
                s = s + t;
            }
        }
        --cur;
        const bool bad = hml_post_bad(s);
        const bool own = cur < hi, is_entry = cur == hi;
#pragma unroll UF
        for (int i = 0; i < KM; ++i)
            if (i < K) {
                const double w = bad ? uni : d[i] / s;
                d[i] = w;
                if (own) a.rows[(uint64_t)cur * K + i] = w;
                if (is_entry) a.entry[(uint64_t)x * K + i] = w;
            }
    }
#pragma unroll UF
    for (int j = 0; j < KM; ++j)
        if (j < K) a.exitv[(uint64_t)x * K + j] = d[j];
}

template <int KM, int DIR>
__device__ __forceinline__ void hml_post_run_chunk(const hml_post_args& a, const double* sA, uint32_t x, const double* from) {
    if (DIR == 0) hml_post_forward_chunk<KM>(a, sA, x, from);
    else hml_post_backward_chunk<KM>(a, sA, x, from);
}

// first pass: a lane per chunk, W blocks of warm-up.  Dynamic LDS: (K K + K) doubles, here and in the two kernels below
template <int KM, int DIR>
HML_KERNEL __launch_bounds__(64) void hml_k_post_first(const hml_post_args a) {
    extern __shared__ double hml_post_lds[];
    hml_post_stage(a, a.par->K, hml_post_lds);
    const uint32_t x = blockIdx.x * 64u + threadIdx.x;
    if (x >= a.n_chunks) return;
    hml_post_run_chunk<KM, DIR>(a, hml_post_lds, x, nullptr);
}

// a repair round: a lane per head (hml_chunk_rerun_walk, over chain indices)
template <int KM, int DIR>
HML_KERNEL __launch_bounds__(64) void hml_k_post_rerun(const hml_post_args a, const uint32_t* __restrict__ heads, uint32_t n_heads,
                                                       const uint8_t* __restrict__ match) {
    extern __shared__ double hml_post_lds[];
    hml_post_stage(a, a.par->K, hml_post_lds);
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n_heads) return;
    auto run = [&](uint32_t x, const double* from) { hml_post_run_chunk<KM, DIR>(a, hml_post_lds, x, from); };
    hml_chunk_rerun_walk(run, a.entry, a.exitv, a.par->K, a.n_chunks, heads[i], match);
}

// what the rounds left: one wavefront (hml_chunk_finish_walk)
template <int KM, int DIR>
HML_KERNEL __launch_bounds__(64) void hml_k_post_finish(const hml_post_args a, const uint8_t* __restrict__ match, unsigned long long* __restrict__ walked) {
    extern __shared__ double hml_post_lds[];
    hml_post_stage(a, a.par->K, hml_post_lds);
    if (blockIdx.x != 0u || blockDim.x != 64u) return;
    auto run = [&](uint32_t x, const double* from) { hml_post_run_chunk<KM, DIR>(a, hml_post_lds, x, from); };
    hml_chunk_finish_walk(run, a.entry, a.exitv, a.par->K, a.n_chunks, match, walked);
}

// a lane per block: gamma_b (stored if asked), the called state and its posterior; degenerate blocks - bad(c_b) - are counted
HML_KERNEL __launch_bounds__(256) void hml_k_post_combine(const double* __restrict__ alpha, const double* __restrict__ beta, const double* __restrict__ cval,
                                                          int K, uint32_t B, double* __restrict__ gamma, int16_t* __restrict__ q, double* __restrict__ conf,
                                                          unsigned long long* __restrict__ n_degenerate) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t b = blockIdx.x * blockDim.x + threadIdx.x; b < B; b += stride) {
        const double* const al = alpha + (uint64_t)b * K;
        const double* const be = beta + (uint64_t)b * K;
        double S = 0.0;
        for (int i = 0; i < K; ++i) S = S + al[i] * be[i];
        const bool bad = hml_post_bad(S);
        int best = 0;
        double top = 0.0;
        for (int i = 0; i < K; ++i) {
            const double g = bad ? al[i] : al[i] * be[i] / S;
            if (gamma) gamma[(uint64_t)b * K + i] = g;
            if (i == 0 || g > top) { top = g; best = i; }
        }
        q[b] = (int16_t)best;
        conf[b] = top;
        if (hml_post_bad(cval[b])) atomicAdd(n_degenerate, 1ull);
    }
}

// one level of the fan-in-64 tree: out[i] = in[64 i] + in[64 i + 1] + ... in this order (the lanes of grid dimension x share it)
__device__ __forceinline__ void hml_post_tree_level(const double* __restrict__ in, uint64_t n, double* __restrict__ out) {
    const uint64_t n_out = (n + 63u) / 64u;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_out; i += stride) {
        const uint64_t lo = 64u * i, hi = lo + 64u < n ? lo + 64u : n;
        double s = in[lo];
        for (uint64_t k = lo + 1u; k < hi; ++k) s = s + in[k];
        out[i] = s;
    }
}
HML_KERNEL __launch_bounds__(256) void hml_k_post_tree(const double* __restrict__ in, uint64_t n, double* __restrict__ out) { hml_post_tree_level(in, n, out); }

// hml_k_seg_run_scatter with the run's confidence: run r starts at position start[i] with state q[i]; every block lowers the
// minimum of its run (words preset to all ones; posteriors are non-negative doubles, ordered as their words are)
HML_KERNEL __launch_bounds__(256) void hml_k_post_run_scatter(const int16_t* __restrict__ q, const double* __restrict__ conf, const uint32_t* __restrict__ start,
                                                              uint32_t M, const int32_t* __restrict__ chunk_base, uint32_t* __restrict__ run_start,
                                                              int16_t* __restrict__ run_state, unsigned long long* run_conf) {
    __shared__ int32_t wsum[4];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int16_t st = i < M ? q[i] : (int16_t)0;
    const int32_t f = (i < M && (i == 0 || st != q[i - 1])) ? 1 : 0;
    int32_t incl = f;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int32_t o = __shfl_up(incl, d);
        if (lane >= d) incl += o;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int32_t pos = chunk_base[blockIdx.x] + incl - f;
    for (int w2 = 0; w2 < wave; ++w2) pos += wsum[w2];
    if (f) { run_start[pos] = start[i]; run_state[pos] = st; }
    if (i < M) {
        const int32_t run = f ? pos : pos - 1;   // (pos counts the heads before i)
        const unsigned long long w = hml_d2u(conf[i]);
        if (w < __hip_atomic_load(run_conf + run, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(run_conf + run, w);
    }
}

#endif

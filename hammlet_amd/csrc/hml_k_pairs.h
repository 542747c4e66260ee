// The pairwise read-outs of the smoothing on the device (hml_posterior_breaks, hml_posterior_regions, include/hml.h), behind a
// smoothing pass that has left alpha and beta in device memory.  hml_pairs_ref.h states the definition and restates it for one
// host thread; DESIGN.md 3c, "pairwise read-outs".
//
//   terms     a lane per block b: p_b, and the 2 K + 1 integer columns pfx_b, cost_b(j), mass_b(j).  A lies in LDS (every lane
//             reads the same word: a broadcast); the emission terms come from the function the decode and the smoothing share (no
//             B K table); adjacent lanes read adjacent rows of alpha and beta.  The columns are stored COLUMN-CONTIGUOUS,
//             col[column][B], so that a wavefront's stores are 64 consecutive words and every scan runs over a contiguous row;
//   scans     inclusive prefix sums of the 2 K + 1 rows, in place, by the three-phase scan of hml_k_scan.h for unsigned long
//             long with the row in the grid's second dimension.  Integers: the sums do not depend on the scan's tree;
//   compact   the boundaries with p_b >= min_prob: flagged and counted per 256 blocks, the counts scanned, then scattered in
//             order - the way hml_k_segment.h forms runs;
//   regions   a lane per region: two binary searches in the block starts, gamma of the two end blocks formed as the smoothing
//             forms it, 2 (2 K + 1) gathered words, and the final doubles by hml_exp_nonpos.
// Memory: (2 K + 2) 8 bytes per block on top of the smoothing's - 96 B per block at K = 5, about 1 KB at K = 64 - and the
// smoothing's c_b, confidences and calls are released before it is taken.
#ifndef HML_K_PAIRS_H
#define HML_K_PAIRS_H

#include "hml_k_posterior.h"
#include "hml_k_scan.h"
#include "hml_pairs_ref.h"   // (HML_PAIRS_COST_CAP, and the host's check of a region)

// llrint(g 2^32) for 0 <= g <= 1
__device__ __forceinline__ unsigned long long hml_pk_fx32(double g) { return (unsigned long long)__double2ll_rn(g * 4294967296.0); }

__device__ __forceinline__ unsigned long long hml_pk_cost(double u, double r) {
    if (hml_post_bad(u) || !(r > 0.0)) return HML_PAIRS_COST_CAP;
    double nl = -hml_log(r);
    nl = nl > 0.0 ? nl : 0.0;
    const unsigned long long q = (unsigned long long)__double2ll_rn(nl * 4194304.0);
    return q < HML_PAIRS_COST_CAP ? q : HML_PAIRS_COST_CAP;
}

// a lane per block.  col[2 K + 1][B]: pfx, cost(0 ... K - 1), mass(0 ... K - 1); p[B]; r[B][K] only for the probe (else null).
// Dynamic LDS: (K K + K) doubles
template <int KM>
HML_KERNEL __launch_bounds__(64) void hml_k_pair_terms(const hml_post_args a, const double* __restrict__ alpha, const double* __restrict__ beta,
                                                       unsigned long long* __restrict__ col, double* __restrict__ p, double* __restrict__ r_out,
                                                       unsigned long long* __restrict__ n_bad) {
    extern __shared__ double hml_post_lds[];
    constexpr int UF = KM <= 16 ? KM : 1;
    const int K = a.par->K;
    hml_post_stage(a, K, hml_post_lds);
    const double* const sA = hml_post_lds;
    const uint64_t B = a.par->B;
    const uint64_t b = (uint64_t)blockIdx.x * 64u + threadIdx.x;
    if (b >= B) return;
    const double* const al = alpha + b * K;
    const double* const be = beta + b * K;
    // mass: n_b fx(gamma_b(j))
    {
        double S = 0.0;
#pragma unroll UF
        for (int i = 0; i < KM; ++i)
            if (i < K) S = S + al[i] * be[i];
        const bool bad = hml_post_bad(S);
        const unsigned long long n = (unsigned long long)(a.starts[b + 1u] - a.starts[b]);
#pragma unroll UF
        for (int i = 0; i < KM; ++i)
            if (i < K) {
                const double g = bad ? al[i] : al[i] * be[i] / S;
                col[(uint64_t)(1 + K + i) * B + b] = n * hml_pk_fx32(g);
            }
    }
    if (b == 0u) {   // no boundary in front of block 0
        col[0] = 0ull;
        p[0] = 0.0;
        for (int j = 0; j < K; ++j) {
            col[(uint64_t)(1 + j) * B] = 0ull;
            if (r_out) r_out[j] = 0.0;
        }
        return;
    }
    float e[KM];
    double v[KM];
    (void)hml_post_terms<KM>(a.par, a.ia, a.starts, (uint32_t)b, e);
#pragma unroll UF
    for (int j = 0; j < KM; ++j)
        if (j < K) v[j] = (double)e[j] * be[j];
    const double* const prev = alpha + (b - 1u) * K;
    double d = 0.0, o = 0.0;
#pragma unroll UF
    for (int i = 0; i < KM; ++i) {
        if (i < K) {
            const double pi_ = prev[i];
            double u = 0.0, diag = 0.0;
#pragma unroll UF
            for (int j = 0; j < KM; ++j)
                if (j < K) {
                    const double aij = sA[i * K + j];
                    u = u + aij * v[j];
                    const double x = (pi_ * aij) * v[j];
                    if (j == i) { d = d + x; diag = aij * v[j]; }
                    else o = o + x;
                }
            const double r = hml_post_bad(u) ? 0.0 : diag / u;
            col[(uint64_t)(1 + i) * B + b] = hml_pk_cost(u, r);
            if (r_out) r_out[b * K + i] = r;
        }
    }
    const double X = d + o;
    const bool bad = hml_post_bad(X);
    const double pb = bad ? 0.0 : o / X;
    p[b] = pb;
    col[b] = hml_pk_fx32(pb);
    if (bad) atomicAdd(n_bad, 1ull);
}

// boundaries b = 1 ... B - 1 with p_b >= min_prob, counted per 256 blocks
HML_KERNEL __launch_bounds__(256) void hml_k_pair_break_count(const double* __restrict__ p, uint32_t B, double min_prob, int32_t* __restrict__ chunk_n) {
    __shared__ int32_t red[4];
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    int32_t f = (i >= 1u && i < B && p[i] >= min_prob) ? 1 : 0;
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) f += __shfl_xor(f, m);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = f;
    __syncthreads();
    if (threadIdx.x == 0) chunk_n[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// scatter, in order: the position starts[b] and p_b of every such boundary
HML_KERNEL __launch_bounds__(256) void hml_k_pair_break_scatter(const double* __restrict__ p, const uint32_t* __restrict__ starts, uint32_t B, double min_prob,
                                                                const int32_t* __restrict__ chunk_base, uint32_t* __restrict__ pos_out,
                                                                double* __restrict__ prob_out) {
    __shared__ int32_t wsum[4];
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double pb = (i >= 1u && i < B) ? p[i] : 0.0;
    const int32_t f = (i >= 1u && i < B && pb >= min_prob) ? 1 : 0;
    int32_t incl = f;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int32_t o = __shfl_up(incl, d);
        if (lane >= d) incl += o;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int32_t at = chunk_base[blockIdx.x] + incl - f;
    for (int w2 = 0; w2 < wave; ++w2) at += wsum[w2];
    if (f) { pos_out[at] = starts[i]; prob_out[at] = pb; }
}

// the last block b of [0, B) with starts[b] <= pos (starts[0] = 0), by one lane
__device__ __forceinline__ uint32_t hml_pk_block_of(const uint32_t* __restrict__ starts, uint32_t B, uint32_t pos) {
    uint32_t lo = 0u, hi = B;   // the answer is in [lo, hi)
    while (hi - lo > 1u) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (starts[mid] <= pos) lo = mid;
        else hi = mid;
    }
    return lo;
}

struct hml_pair_regions_out {
    double *whole, *whole_state, *expected_breaks, *share;   // [n], [n][K], [n], [n][K]
    unsigned long long* raw;                                 // [n][2 K + 1]
};

// a lane per region (every region is valid: the host has refused the others); col holds the inclusive prefix sums
HML_KERNEL __launch_bounds__(256) void hml_k_pair_regions(const uint32_t* __restrict__ starts, uint32_t B, int K, const double* __restrict__ alpha,
                                                          const double* __restrict__ beta, const unsigned long long* __restrict__ col,
                                                          const uint32_t* __restrict__ rg_start, const uint32_t* __restrict__ rg_end, uint64_t n,
                                                          hml_pair_regions_out out) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += stride) {
        const uint32_t st = rg_start[r], en = rg_end[r];
        const uint32_t ba = hml_pk_block_of(starts, B, st), be = hml_pk_block_of(starts, B, en - 1u);
        const unsigned long long nb = col[be] - col[ba];
        const unsigned long long cut_a = (unsigned long long)(st - starts[ba]), cut_e = (unsigned long long)(starts[be + 1u] - en);
        const double len = (double)(en - st);
        const double* const al_a = alpha + (uint64_t)ba * K;
        const double* const be_a = beta + (uint64_t)ba * K;
        const double* const al_e = alpha + (uint64_t)be * K;
        const double* const be_e = beta + (uint64_t)be * K;
        double Sa = 0.0, Se = 0.0;
        for (int i = 0; i < K; ++i) { Sa = Sa + al_a[i] * be_a[i]; Se = Se + al_e[i] * be_e[i]; }
        const bool bad_a = hml_post_bad(Sa), bad_e = hml_post_bad(Se);
        unsigned long long* const raw = out.raw + r * (uint64_t)(2 * K + 1);
        raw[0] = nb;
        out.expected_breaks[r] = (double)nb * (1.0 / 4294967296.0);
        double whole = 0.0;
        for (int j = 0; j < K; ++j) {
            const double ga = bad_a ? al_a[j] : al_a[j] * be_a[j] / Sa;
            const double ge = bad_e ? al_e[j] : al_e[j] * be_e[j] / Se;
            const unsigned long long* const C = col + (uint64_t)(1 + j) * B;
            const unsigned long long* const G = col + (uint64_t)(1 + K + j) * B;
            const unsigned long long dc = C[be] - C[ba];
            const double ws = ga * hml_exp_nonpos(-(double)dc * (1.0 / 4194304.0));
            out.whole_state[r * K + j] = ws;
            whole = whole + ws;
            const unsigned long long m = G[be] - (ba ? G[ba - 1u] : 0ull) - cut_a * hml_pk_fx32(ga) - cut_e * hml_pk_fx32(ge);
            out.share[r * K + j] = ((double)m * (1.0 / 4294967296.0)) / len;
            raw[1 + j] = dc;
            raw[1 + K + j] = m;
        }
        out.whole[r] = whole;
    }
}

#endif

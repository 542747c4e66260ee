// The E-step's expected counts on the device (hml_expected_counts, include/hml.h), behind a smoothing pass that has left alpha and
// beta in device memory.  hml_em_ref.h states the definition and restates it for one host thread; DESIGN.md 3c, "EM".
//
// Every result is the fan-in-64 tree sum of one COLUMN of per-block terms, the K K columns xi(i, j) over the B - 1 blocks
// b = 1 ... B - 1 (leaf b - 1) and the K (2 + 2 D) columns occ, stay, sx, sxx over the B blocks (leaf b): the two trees' groups
// of 64 lie one block apart.  The order of additions per column is the definition's; which lane adds is free:
//   norm     a lane per block b >= 1: X_b, its K K additions in the prescribed order (i outer, j inner), stored per block;
//   reduce   a workgroup per group g of 64 leaves, of both trees at once: blocks 64 g ... 64 g + 64.  In tiles of 16 leaves it
//            stages the rows alpha_{base+l} (alpha_{b-1} of xi's leaf l and alpha of the other columns' leaf l), beta, v_b =
//            e_b beta_b (the emission terms computed here, by the function the decode and the smoothing share: no B K table),
//            gamma, n_b and the block's sums, then a lane per column makes the 16 in-order additions of its column; a lane
//            keeps its columns' running sums (up to 19 at K = 64, D = 4) and its A_ij in registers across the four tiles;
//            For K <= 16 that shape leaves most lanes idle (45 columns at K = 5): hml_k_em_reduce_small is one wavefront per group,
//            a lane per block while staging - X_b included, so `norm` is not launched - and all 64 leaves in one tile;
//   tree     the upper levels, a lane per value of the next level over all columns at once (hml_k_post_tree's loop).
// Partials: level 1 is ceil(B / 64) rows of K K + K (2 + 2 D) doubles (column-contiguous, so that stores and the next level's
// loads are coalesced), level 2 a 64th of that; the levels above alternate between the two.
#ifndef HML_K_EM_H
#define HML_K_EM_H

#include "hml_k_posterior.h"

#define HML_EM_TL 16   // leaves a tile
#define HML_EM_NQ 19   // columns a lane of 256 at the most: ceil((64 64 + 64 (2 + 2 4)) / 256)

// X_b for b = 1 ... B - 1 (X[0] is not written); blocks with bad(X_b) are counted.  Dynamic LDS: (K K + K) doubles
template <int KM>
__device__ __forceinline__ void hml_em_norm_block(const hml_post_args& a, const double* sA, const double* __restrict__ alpha, const double* __restrict__ beta,
                                                  double* __restrict__ X, unsigned long long* __restrict__ n_bad) {
    constexpr int UF = KM <= 16 ? KM : 1;
    const int K = a.par->K;
    const uint64_t b64 = (uint64_t)blockIdx.x * 64u + threadIdx.x + 1u;
    if (b64 >= (uint64_t)a.par->B) return;
    const uint32_t b = (uint32_t)b64;
    float e[KM];
    double v[KM];
    (void)hml_post_terms<KM>(a.par, a.ia, a.starts, b, e);
#pragma unroll UF
    for (int j = 0; j < KM; ++j)
        if (j < K) v[j] = (double)e[j] * beta[(uint64_t)b * K + j];
    double s = 0.0;
#pragma unroll UF
    for (int i = 0; i < KM; ++i) {
        if (i < K) {
            const double al = alpha[(uint64_t)(b - 1u) * K + i];
#pragma unroll UF
            for (int j = 0; j < KM; ++j)
                if (j < K) s = s + (al * sA[i * K + j]) * v[j];
        }
    }
    X[b] = s;
    if (hml_post_bad(s)) atomicAdd(n_bad, 1ull);
}
template <int KM>
HML_KERNEL __launch_bounds__(64) void hml_k_em_norm(const hml_post_args a, const double* __restrict__ alpha, const double* __restrict__ beta,
                                                    double* __restrict__ X, unsigned long long* __restrict__ n_bad) {
    extern __shared__ double hml_post_lds[];
    hml_post_stage(a, a.par->K, hml_post_lds);
    hml_em_norm_block<KM>(a, hml_post_lds, alpha, beta, X, n_bad);
}

struct hml_em_args {
    const hml_vit_par* par;
    const double* A;             // [K][K] widened
    const float2* ia;
    const uint32_t* starts;
    const double *alpha, *beta;  // [B][K]
    const double* X;             // [B]
    double* part;                // [ceil(B / 64)][ncols]: level 1
    double* first;               // [K]: gamma_0
};

// level 1 of every column's tree: workgroup g owns leaves 64 g ... 64 g + 63 of both trees.  Column order: xi row-major, then
// occ[K], stay[K], sx[D][K], sxx[D][K]
__device__ __forceinline__ void hml_em_reduce_group(const hml_em_args& a) {
    __shared__ double sAl[HML_EM_TL][HML_CAP_K], sBe[HML_EM_TL + 1][HML_CAP_K], sV[HML_EM_TL][HML_CAP_K], sG[HML_EM_TL][HML_CAP_K];
    __shared__ float sE[HML_EM_TL][HML_CAP_K];
    __shared__ double sX[HML_EM_TL], sN[HML_EM_TL], sS[HML_EM_TL][2 * HML_MAX_D];
    const hml_vit_par* const par = a.par;
    const int tid = threadIdx.x, K = par->K, D = par->D, KK = K * K;
    const int ncols = KK + K * (2 + 2 * D);
    const uint64_t B = par->B;
    const uint64_t base0 = (uint64_t)blockIdx.x * 64u;
    double acc[HML_EM_NQ], Aq[HML_EM_NQ];
#pragma unroll
    for (int q = 0; q < HML_EM_NQ; ++q) {
        const int col = tid + 256 * q;
        Aq[q] = col < KK ? a.A[col] : 0.0;
        acc[q] = 0.0;
    }
    for (int t = 0; t < 64 / HML_EM_TL; ++t) {
        const uint64_t base = base0 + (uint64_t)(t * HML_EM_TL);
        if (base >= B) break;
        // the rows alpha_{base + l} (l < TL) and beta_{base + l} (l <= TL)
        for (int idx = tid; idx < (HML_EM_TL + 1) * K; idx += 256) {
            const int l = idx / K, i = idx - l * K;
            const uint64_t blk = base + (uint64_t)l;
            if (blk < B) {
                sBe[l][i] = a.beta[blk * K + i];
                if (l < HML_EM_TL) sAl[l][i] = a.alpha[blk * K + i];
            }
        }
        __syncthreads();
        if (tid < HML_EM_TL) {
            // xi's leaf l is block b = base + l + 1: v_b = e_b beta_b, and X_b
            const int l = tid;
            const uint64_t b = base + (uint64_t)l + 1u;
            if (b < B) {
                hml_vit_block blk;
                hml_vit_block_load(par, a.ia, a.starts, (uint32_t)b, blk);
                float top = -3.40282346638528859812e+38f;
                for (int j = 0; j < K; ++j) {
                    const float v = hml_vit_emit_float(par, blk, j);
                    sE[l][j] = v;
                    top = (v < top) ? top : v;
                }
                for (int j = 0; j < K; ++j) sV[l][j] = (double)hml_expf(sE[l][j] - top) * sBe[l + 1][j];
                sX[l] = a.X[b];
            }
        } else if (tid >= 64 && tid < 64 + HML_EM_TL) {
            // the other columns' leaf l is block b = base + l: gamma_b, n_b and the block's sums
            const int l = tid - 64;
            const uint64_t b = base + (uint64_t)l;
            if (b < B) {
                double S = 0.0;
                for (int i = 0; i < K; ++i) S = S + sAl[l][i] * sBe[l][i];
                const bool bad = hml_post_bad(S);
                for (int i = 0; i < K; ++i) {
                    const double g = bad ? sAl[l][i] : sAl[l][i] * sBe[l][i] / S;
                    sG[l][i] = g;
                    if (b == 0u) a.first[i] = g;
                }
                hml_vit_block blk;
                hml_vit_block_load(par, a.ia, a.starts, (uint32_t)b, blk);
                sN[l] = (double)(a.starts[b + 1u] - a.starts[b]);
                for (int d = 0; d < D; ++d) { sS[l][d] = (double)blk.sx[d]; sS[l][D + d] = (double)blk.sq[d]; }
            }
        }
        __syncthreads();
        const uint64_t left = B - base;   // >= 1
        const int n_o = left < (uint64_t)HML_EM_TL ? (int)left : HML_EM_TL;
        const int n_x = left - 1u < (uint64_t)HML_EM_TL ? (int)(left - 1u) : HML_EM_TL;
#pragma unroll
        for (int q = 0; q < HML_EM_NQ; ++q) {
            const int col = tid + 256 * q;
            if (col < ncols) {
                double s = acc[q];
                if (col < KK) {
                    const int i = col / K, j = col - i * K;
                    const double aij = Aq[q];
                    for (int l = 0; l < n_x; ++l) {
                        const double X = sX[l];
                        const double val = hml_post_bad(X) ? 0.0 : ((sAl[l][i] * aij) * sV[l][j]) / X;
                        s = (t == 0 && l == 0) ? val : s + val;
                    }
                } else {
                    const int c2 = col - KK, kind = c2 / K, j = c2 - kind * K;
                    for (int l = 0; l < n_o; ++l) {
                        const double g = sG[l][j];
                        double val;
                        if (kind == 0) val = sN[l] * g;
                        else if (kind == 1) val = (sN[l] - 1.0) * g;
                        else val = g * sS[l][kind - 2];
                        s = (t == 0 && l == 0) ? val : s + val;
                    }
                }
                acc[q] = s;
            }
        }
        __syncthreads();
    }
    const bool has_x = base0 + 1u < B;   // the group holds a leaf of xi's tree
#pragma unroll
    for (int q = 0; q < HML_EM_NQ; ++q) {
        const int col = tid + 256 * q;
        if (col < ncols && (col >= KK || has_x)) a.part[(uint64_t)blockIdx.x * ncols + col] = acc[q];
    }
}
HML_KERNEL __launch_bounds__(256) void hml_k_em_reduce(const hml_em_args a) { hml_em_reduce_group(a); }

// The same level 1 for K <= KS <= 16, where the shape above leaves most lanes without a column: ONE WAVEFRONT per group, all 64
// leaves in one tile.  While staging, lane l owns block base + l: it reads alpha_b and beta_b (adjacent lanes adjacent rows), stores
// gamma_b, n_b and the block's sums, then for xi's leaf l - block b + 1, whose alpha_{b-1} it holds in registers - the emission
// terms, v and X_{b+1} with its K K additions in the prescribed order (A in LDS), so hml_k_em_norm and the array X are not needed;
// then a lane per column makes the 64 in-order additions.  Rows are padded to KS + 1 doubles against bank conflicts.
template <int KS>
__device__ __forceinline__ void hml_em_reduce_small_group(const hml_em_args& a, unsigned long long* __restrict__ n_bad) {
    constexpr int NQ = (KS * KS + KS * (2 + 2 * HML_MAX_D) + 63) / 64;
    __shared__ double sA[KS * KS], sAl[64][KS + 1], sV[64][KS + 1], sG[64][KS + 1];
    __shared__ double sX[64], sN[64], sS[64][2 * HML_MAX_D + 1];
    const hml_vit_par* const par = a.par;
    const int l = threadIdx.x, K = par->K, D = par->D, KK = K * K;
    const int ncols = KK + K * (2 + 2 * D);
    const uint64_t B = par->B;
    const uint64_t base = (uint64_t)blockIdx.x * 64u;
    for (int i = l; i < KK; i += 64) sA[i] = a.A[i];
    __syncthreads();
    const uint64_t bo = base + (uint64_t)l, bx = bo + 1u;
    if (bo < B) {
        double al[KS], be[KS];
        double S = 0.0;
#pragma unroll
        for (int i = 0; i < KS; ++i)
            if (i < K) {
                al[i] = a.alpha[bo * K + i];
                be[i] = a.beta[bo * K + i];
                S = S + al[i] * be[i];
                sAl[l][i] = al[i];
            }
        const bool bad = hml_post_bad(S);
#pragma unroll
        for (int i = 0; i < KS; ++i)
            if (i < K) {
                const double g = bad ? al[i] : al[i] * be[i] / S;
                sG[l][i] = g;
                if (bo == 0u) a.first[i] = g;
            }
        hml_vit_block blk;
        hml_vit_block_load(par, a.ia, a.starts, (uint32_t)bo, blk);
        sN[l] = (double)(a.starts[bo + 1u] - a.starts[bo]);
        for (int d = 0; d < D; ++d) { sS[l][d] = (double)blk.sx[d]; sS[l][D + d] = (double)blk.sq[d]; }
        if (bx < B) {
            float e[KS];
            double v[KS];
            (void)hml_post_terms<KS>(par, a.ia, a.starts, (uint32_t)bx, e);
#pragma unroll
            for (int j = 0; j < KS; ++j)
                if (j < K) {
                    v[j] = (double)e[j] * a.beta[bx * K + j];
                    sV[l][j] = v[j];
                }
            double X = 0.0;
#pragma unroll
            for (int i = 0; i < KS; ++i) {
                if (i < K) {
#pragma unroll
                    for (int j = 0; j < KS; ++j)
                        if (j < K) X = X + (al[i] * sA[i * K + j]) * v[j];
                }
            }
            sX[l] = X;
            if (hml_post_bad(X)) atomicAdd(n_bad, 1ull);
        }
    }
    __syncthreads();
    const uint64_t left = B - base;   // >= 1
    const int n_o = left < 64u ? (int)left : 64;
    const int n_x = left - 1u < 64u ? (int)(left - 1u) : 64;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const int col = l + 64 * q;
        if (col >= ncols) continue;
        double s = 0.0;
        if (col < KK) {
            if (n_x == 0) continue;   // the group holds no leaf of xi's tree
            const int i = col / K, j = col - i * K;
            const double aij = sA[col];
            for (int k = 0; k < n_x; ++k) {
                const double X = sX[k];
                const double val = hml_post_bad(X) ? 0.0 : ((sAl[k][i] * aij) * sV[k][j]) / X;
                s = k == 0 ? val : s + val;
            }
        } else {
            const int c2 = col - KK, kind = c2 / K, j = c2 - kind * K;
            for (int k = 0; k < n_o; ++k) {
                const double g = sG[k][j];
                double val;
                if (kind == 0) val = sN[k] * g;
                else if (kind == 1) val = (sN[k] - 1.0) * g;
                else val = g * sS[k][kind - 2];
                s = k == 0 ? val : s + val;
            }
        }
        a.part[(uint64_t)blockIdx.x * ncols + col] = s;
    }
}
template <int KS>
HML_KERNEL __launch_bounds__(64) void hml_k_em_reduce_small(const hml_em_args a, unsigned long long* __restrict__ n_bad) { hml_em_reduce_small_group<KS>(a, n_bad); }

// one level of all columns' trees: rows of ncols values; the first KK columns have n_x rows, the others n_o >= n_x
__device__ __forceinline__ void hml_em_tree_level(const double* __restrict__ in, uint64_t n_x, uint64_t n_o, uint32_t ncols, uint32_t KK,
                                                  double* __restrict__ out) {
    const uint64_t total = ((n_o + 63u) / 64u) * ncols;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += stride) {
        const uint64_t i = idx / ncols;
        const uint32_t col = (uint32_t)(idx - i * ncols);
        const uint64_t n = col < KK ? n_x : n_o;
        const uint64_t lo = 64u * i, hi = lo + 64u < n ? lo + 64u : n;
        if (lo >= n) continue;
        double s = in[lo * ncols + col];
        for (uint64_t k = lo + 1u; k < hi; ++k) s = s + in[k * ncols + col];
        out[i * ncols + col] = s;
    }
}
HML_KERNEL __launch_bounds__(256) void hml_k_em_tree(const double* __restrict__ in, uint64_t n_x, uint64_t n_o, uint32_t ncols, uint32_t KK,
                                                     double* __restrict__ out) { hml_em_tree_level(in, n_x, n_o, ncols, KK, out); }

#endif

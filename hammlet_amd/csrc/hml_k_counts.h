// The count read-outs of the smoothing on the device (hml_posterior_region_counts, hml_posterior_count_terms, include/hml.h),
// behind a smoothing pass that has left alpha and beta in device memory.  hml_counts_ref.h states the definition and restates
// it for one host thread; DESIGN.md 3c, "count read-outs".
//
//   terms     a lane per block b, as hml_k_pair_terms: A in LDS (a broadcast), the emission terms from the function the decode
//             and the smoothing share, v_b and rho_b stored as rows [B][K], the pairs (b, i) without a usable u_b(i) counted;
//   count walk   one wavefront - a workgroup of 64 - per region, grid-stride over the regions.  The K (H + 1) cells lie in
//             LDS as f[h][j]; lane l owns the cells l, l + 64, ...  Per block the lanes 0 ... K - 1 load v_b and rho_b (adjacent
//             lanes, adjacent words; the next block's are in flight while this one is computed), every lane forms its cells in
//             registers between two workgroup barriers and stores them back: one cell buffer.  The lanes of one h and adjacent
//             j read the same cell of the old buffer (a broadcast) and adjacent words of A's row (no bank conflict);
//   avoidance walk   the same shape over the cells g[x][i], the struck-out state x in slices of at most 16 states along the
//             grid's second dimension: a workgroup holds at most 16 K cells.
// Every cell's sum is formed by one lane in the order the header states: no cross-lane reduction, so no word can depend on the
// launch geometry.  LDS: (K K + K) + 2 K + cells doubles - at most 32.5 KB + 1 KB + 8 KB at 64 states, well inside 64 KB.  A lane
// holds at most 1024 / 64 = 16 cells.  More than 32 states are served, not tuned: A alone then takes 8 ... 32 KB of a
// workgroup's LDS and few wavefronts share a compute unit.
// Memory: 2 K 8 bytes per block on top of the smoothing's; c_b, confidences and calls are released before it is taken.
#ifndef HML_K_COUNTS_H
#define HML_K_COUNTS_H

#include "hml_k_pairs.h"     // (hml_pk_block_of; it brings hml_k_posterior.h)
#include "hml_counts_ref.h"  // (the limits, and the host's check of max_breaks)

#define HML_COUNTS_LANE_CELLS (HML_COUNTS_MAX_CELLS / 64u)   // 16

// the walks are compiled for 1, 2, 4, 8 and 16 cells a lane, so that a few cells do not cost the registers of many: the least of
// them that holds `cells`
static inline int hml_counts_lane_cells(int cells) {
    int nc = 1;
    while (64 * nc < cells) nc *= 2;
    return nc;
}

// a lane per block.  v[B][K], rho[B][K].  Dynamic LDS: (K K + K) doubles
template <int KM>
HML_KERNEL __launch_bounds__(64) void hml_k_count_terms(const hml_post_args a, const double* __restrict__ beta, double* __restrict__ v_out, double* __restrict__ rho_out,
                                                        unsigned long long* __restrict__ n_bad) {
    extern __shared__ double hml_post_lds[];
    constexpr int UF = KM <= 16 ? KM : 1;
    const int K = a.par->K;
    hml_post_stage(a, K, hml_post_lds);
    const double* const sA = hml_post_lds;
    const uint64_t B = a.par->B;
    const uint64_t b = (uint64_t)blockIdx.x * 64u + threadIdx.x;
    if (b >= B) return;
    if (b == 0u) {   // no boundary in front of block 0
        for (int j = 0; j < K; ++j) { v_out[j] = 0.0; rho_out[j] = 0.0; }
        return;
    }
    const double* const be = beta + b * K;
    float e[KM];
    double v[KM];
    (void)hml_post_terms<KM>(a.par, a.ia, a.starts, (uint32_t)b, e);
#pragma unroll UF
    for (int j = 0; j < KM; ++j)
        if (j < K) {
            v[j] = (double)e[j] * be[j];
            v_out[b * K + j] = hml_counts_v_kept(v[j]);   // (u is formed from v itself)
        }
    unsigned long long bad = 0ull;
#pragma unroll UF
    for (int i = 0; i < KM; ++i) {
        if (i < K) {
            double u = 0.0;
#pragma unroll UF
            for (int j = 0; j < KM; ++j)
                if (j < K) u = u + sA[i * K + j] * v[j];
            const bool ok = hml_counts_u_ok(u);
            bad += ok ? 0ull : 1ull;
            rho_out[b * K + i] = ok ? 1.0 / u : 0.0;
        }
    }
    if (bad) atomicAdd(n_bad, bad);
}

// gamma_b(j) as the smoothing forms it, the whole sum by the calling lane
__device__ __forceinline__ double hml_ck_gamma(const double* __restrict__ al, const double* __restrict__ be, int K, int j) {
    double S = 0.0;
    for (int i = 0; i < K; ++i) S = S + al[i] * be[i];
    return hml_post_bad(S) ? al[j] : al[j] * be[j] / S;
}

struct hml_count_walk_args {
    const double *alpha, *beta, *v, *rho;     // [B][K] each
    const uint32_t *rg_start, *rg_end;        // [n]: valid regions (the host has refused the others)
    uint64_t n;
    uint32_t H;
    double *hist, *whole_state, *avoid;       // [n][H + 1], [n][K], [n][K]
    unsigned long long* info;                 // [0] the sum of be - ba over the regions, [1] the largest (count walk only)
};

// One workgroup of 64 per region, grid-stride; NC: the cells a lane holds at the most, K (H + 1) <= 64 NC (hml_counts_lane_cells).
// Dynamic LDS: (K K + K) + 2 K + K (H + 1) doubles
template <int NC>
HML_KERNEL __launch_bounds__(64) void hml_k_count_walk(const hml_post_args a, const hml_count_walk_args w) {
    extern __shared__ double hml_post_lds[];
    const int K = a.par->K;
    const uint32_t B = a.par->B;
    hml_post_stage(a, K, hml_post_lds);
    const double* const sA = hml_post_lds;
    double* const sV = hml_post_lds + K * K + K;
    double* const sR = sV + K;
    double* const sF = sR + K;   // f[h][j]
    const int lane = threadIdx.x;
    const int H = (int)w.H, cells = K * (H + 1);
    int cj[NC], ch[NC];
#pragma unroll
    for (int m = 0; m < NC; ++m) {
        const int c = lane + 64 * m;
        ch[m] = c / K;
        cj[m] = c - ch[m] * K;
    }
    for (uint64_t r = blockIdx.x; r < w.n; r += gridDim.x) {
        const uint32_t st = w.rg_start[r], en = w.rg_end[r];
        const uint32_t ba = hml_pk_block_of(a.starts, B, st), be = hml_pk_block_of(a.starts, B, en - 1u);
        if (lane == 0) {
            atomicAdd(w.info, (unsigned long long)(be - ba));
            atomicMax(w.info + 1, (unsigned long long)(be - ba));
        }
        __syncthreads();   // (the read-out of the region before this one is over)
#pragma unroll
        for (int m = 0; m < NC; ++m) {
            const int c = lane + 64 * m;
            if (c < cells) sF[c] = ch[m] == 0 ? hml_ck_gamma(w.alpha + (uint64_t)ba * K, w.beta + (uint64_t)ba * K, K, cj[m]) : 0.0;
        }
        double nv = 0.0, nr = 0.0;   // v and rho of the block to come, lanes 0 ... K - 1
        if (lane < K && ba < be) { nv = w.v[(uint64_t)(ba + 1u) * K + lane]; nr = w.rho[(uint64_t)(ba + 1u) * K + lane]; }
        for (uint32_t b = ba + 1u; b <= be; ++b) {
            if (lane < K) { sV[lane] = nv; sR[lane] = nr; }
            __syncthreads();
            if (lane < K && b < be) { nv = w.v[(uint64_t)(b + 1u) * K + lane]; nr = w.rho[(uint64_t)(b + 1u) * K + lane]; }
            double nf[NC];
#pragma unroll
            for (int m = 0; m < NC; ++m) {
                const int c = lane + 64 * m;
                if (c < cells) {
                    const int j = cj[m], h = ch[m];
                    double s = 0.0;
                    if (h >= 1) {
                        const double* const lo = sF + (h - 1) * K;
                        const double* const up = sF + h * K;
                        for (int i = 0; i < K; ++i) {
                            if (i == j) continue;
                            double src = lo[i] * sR[i];
                            if (h == H) src = src + up[i] * sR[i];
                            s = s + sA[i * K + j] * src;
                        }
                    }
                    nf[m] = (sA[j * K + j] * (sF[c] * sR[j]) + s) * sV[j];
                }
            }
            __syncthreads();
#pragma unroll
            for (int m = 0; m < NC; ++m) {
                const int c = lane + 64 * m;
                if (c < cells) sF[c] = nf[m];
            }
        }
        __syncthreads();
        if (lane <= H) {
            double s = 0.0;
            for (int j = 0; j < K; ++j) s = s + sF[lane * K + j];
            w.hist[r * (uint64_t)(H + 1) + lane] = s;
        }
        if (lane < K) w.whole_state[r * (uint64_t)K + lane] = sF[lane];
    }
}

// The same over g[x][i] for the struck-out states x = 16 blockIdx.y ... of this slice, min(K, 16) K <= 64 NC.
// Dynamic LDS: (K K + K) + 2 K + 16 K doubles
template <int NC>
HML_KERNEL __launch_bounds__(64) void hml_k_count_avoid(const hml_post_args a, const hml_count_walk_args w) {
    extern __shared__ double hml_post_lds[];
    const int K = a.par->K;
    const uint32_t B = a.par->B;
    hml_post_stage(a, K, hml_post_lds);
    const double* const sA = hml_post_lds;
    double* const sV = hml_post_lds + K * K + K;
    double* const sR = sV + K;
    double* const sG = sR + K;   // g[x - x0][i]
    const int lane = threadIdx.x;
    const int x0 = (int)blockIdx.y * HML_COUNTS_SLICE;
    const int nx = K - x0 < HML_COUNTS_SLICE ? K - x0 : HML_COUNTS_SLICE;
    const int cells = nx * K;
    int ci[NC], cx[NC];
#pragma unroll
    for (int m = 0; m < NC; ++m) {
        const int c = lane + 64 * m;
        cx[m] = c / K;
        ci[m] = c - cx[m] * K;
    }
    for (uint64_t r = blockIdx.x; r < w.n; r += gridDim.x) {
        const uint32_t st = w.rg_start[r], en = w.rg_end[r];
        const uint32_t ba = hml_pk_block_of(a.starts, B, st), be = hml_pk_block_of(a.starts, B, en - 1u);
        __syncthreads();   // (the read-out of the region before this one is over)
#pragma unroll
        for (int m = 0; m < NC; ++m) {
            const int c = lane + 64 * m;
            if (c < cells) sG[c] = ci[m] == x0 + cx[m] ? 0.0 : hml_ck_gamma(w.alpha + (uint64_t)ba * K, w.beta + (uint64_t)ba * K, K, ci[m]);
        }
        double nv = 0.0, nr = 0.0;
        if (lane < K && ba < be) { nv = w.v[(uint64_t)(ba + 1u) * K + lane]; nr = w.rho[(uint64_t)(ba + 1u) * K + lane]; }
        for (uint32_t b = ba + 1u; b <= be; ++b) {
            if (lane < K) { sV[lane] = nv; sR[lane] = nr; }
            __syncthreads();
            if (lane < K && b < be) { nv = w.v[(uint64_t)(b + 1u) * K + lane]; nr = w.rho[(uint64_t)(b + 1u) * K + lane]; }
            double ng[NC];
#pragma unroll
            for (int m = 0; m < NC; ++m) {
                const int c = lane + 64 * m;
                if (c < cells) {
                    const int i = ci[m], x = x0 + cx[m];
                    const double* const row = sG + cx[m] * K;
                    double s = 0.0;
                    for (int k = 0; k < K; ++k) {
                        if (k == x) continue;
                        s = s + sA[k * K + i] * (row[k] * sR[k]);
                    }
                    ng[m] = i == x ? 0.0 : s * sV[i];
                }
            }
            __syncthreads();
#pragma unroll
            for (int m = 0; m < NC; ++m) {
                const int c = lane + 64 * m;
                if (c < cells) sG[c] = ng[m];
            }
        }
        __syncthreads();
        if (lane < nx) {
            const int x = x0 + lane;
            double s = 0.0;
            for (int i = 0; i < K; ++i)
                if (i != x) s = s + sG[lane * K + i];
            w.avoid[r * (uint64_t)K + x] = s;
        }
    }
}

#endif

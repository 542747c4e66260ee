// Per-position agreement of n chains on the emission level: the Gelman-Rubin potential scale reduction (R-hat) from the chains'
// recorded levels (hml_k_levels.h), per segment of the UNION of the chains' level boundaries (include/hml.h,
// hml_levels_agreement_rle; DESIGN.md section 3c'''').  Nothing here walks the T positions: the chains' boundary bitmaps are
// ORed word by word (hml_k_agree_or), the union's starts are compacted like any bitmap's (hml_k_marg_count / hml_k_marg_scatter),
// and a chain's own segment under a union segment is found by RANK - a chain's starts are a subset of the union's, so the
// number of the chain's starts up to a union start, minus one, is the chain's segment there (hml_k_agree_flags, then the fixed
// scan of hml_k_scan.h over each chain's row of flags).  The contexts are only read.
#ifndef HML_K_AGREE_H
#define HML_K_AGREE_H

#include "hml_math.h"
#include "hml_state.h"

#define HML_AGREE_MAX_CHAINS 64

// what the kernels read of the n chains, passed by value: the boundary bitmap of each chain's levels, its inclusive segment
// sums sum[2 D][M] (gather_level_segments: the bits hml_levels_rle returns) and its number of segments M
struct hml_agree_chains {
    const uint32_t* boundary[HML_AGREE_MAX_CHAINS];
    const double* sum[HML_AGREE_MAX_CHAINS];
    uint32_t M[HML_AGREE_MAX_CHAINS];
};

// out[w] = the OR over the chains of boundary[c][w], for the `words` words of a bitmap
HML_KERNEL __launch_bounds__(256) void hml_k_agree_or(hml_agree_chains ch, int n, uint32_t words, uint32_t* __restrict__ out) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t w = blockIdx.x * blockDim.x + threadIdx.x; w < words; w += stride) {
        uint32_t bits = 0u;
        for (int c = 0; c < n; ++c) bits |= ch.boundary[c][w];
        out[w] = bits;
    }
}

// flag[c][i] = 1 iff chain c has a boundary at union start i (position 0 always is one, as in hml_k_marg_count)
HML_KERNEL __launch_bounds__(256) void hml_k_agree_flags(hml_agree_chains ch, int n, const uint32_t* __restrict__ useg, uint32_t U,
                                                         uint8_t* __restrict__ flag) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < U; i += stride) {
        const uint32_t t = useg[i];
        for (int c = 0; c < n; ++c)
            flag[(uint64_t)c * U + i] = (t == 0u) ? (uint8_t)1 : (uint8_t)((ch.boundary[c][t >> 5] >> (t & 31u)) & 1u);
    }
}

// One thread per union segment.  rank[c][i]: the inclusive scan of flag[c][.], so chain c's segment under union segment i is
// rank - 1.  Per dimension d, in double, in this order (no contraction), the sums over the chains from chain 0 upward from 0.0:
//   m_c = S1_c / N;  q_c = S2_c / N - m_c * m_c, 0 unless q_c > 0;  w0 = (sum q_c) / n;  mbar = (sum m_c) / n;
//   between = (sum (m_c - mbar) * (m_c - mbar)) / (n - 1);  within = w0 * (N / (N - 1));
//   rhat = sqrt((w0 + between) / within) if within > 0, else 1 if between == 0, else +infinity.
// within, between, rhat: [D][U] doubles; rhat_f: rhat rounded once to float (the dense form's rows).
HML_KERNEL __launch_bounds__(256) void hml_k_agree_eval(hml_agree_chains ch, int n, int D, const uint32_t* __restrict__ rank, uint32_t U,
                                                        unsigned long long n_recorded, double* __restrict__ within,
                                                        double* __restrict__ between, double* __restrict__ rhat, float* __restrict__ rhat_f) {
    const uint32_t stride = gridDim.x * blockDim.x;
    const double N = (double)n_recorded;
    const double nn = (double)n;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < U; i += stride) {
        for (int d = 0; d < D; ++d) {
            double sq = 0.0, sm = 0.0;
            for (int c = 0; c < n; ++c) {
                const uint32_t Mc = ch.M[c];
                uint32_t j = rank[(uint64_t)c * U + i] - 1u;
                if (j >= Mc) j = Mc - 1u;   // (cannot happen: the chain's starts are among the union's; never read out of bounds)
                const double m = ch.sum[c][(uint64_t)(2 * d) * Mc + j] / N;
                double q = ch.sum[c][(uint64_t)(2 * d + 1) * Mc + j] / N - m * m;
                if (!(q > 0.0)) q = 0.0;
                sq += q;
                sm += m;
            }
            const double w0 = sq / nn;
            const double mbar = sm / nn;
            double sb = 0.0;
            for (int c = 0; c < n; ++c) {   // (the same quotient again: the same bits as m above)
                const uint32_t Mc = ch.M[c];
                uint32_t j = rank[(uint64_t)c * U + i] - 1u;
                if (j >= Mc) j = Mc - 1u;
                const double m = ch.sum[c][(uint64_t)(2 * d) * Mc + j] / N;
                sb += (m - mbar) * (m - mbar);
            }
            const double b = sb / (nn - 1.0);
            const double w = w0 * (N / (N - 1.0));
            double r;
            if (w > 0.0) r = HML_SQRT((w0 + b) / w);
            else r = (b == 0.0) ? 1.0 : __builtin_inf();
            const uint64_t o = (uint64_t)d * U + i;
            within[o] = w;
            between[o] = b;
            rhat[o] = r;
            rhat_f[o] = (float)r;
        }
    }
}

// The summary's first stage: per workgroup and dimension, over the union segments the workgroup takes, the positions (segment
// lengths, 64-bit integers: exact) with rhat > threshold - +infinity included - and with rhat == +infinity, and the largest
// finite rhat (0 if none).  part_cnt[(block * D + d) * 2 + {0, 1}], part_max[block * D + d]; the host adds the partials.
HML_KERNEL __launch_bounds__(256) void hml_k_agree_summary(const double* __restrict__ rhat, const uint32_t* __restrict__ useg, uint32_t U,
                                                           uint32_t T, int D, double threshold, unsigned long long* __restrict__ part_cnt,
                                                           double* __restrict__ part_max) {
    __shared__ unsigned long long sh_above[4], sh_inf[4];
    __shared__ double sh_max[4];
    const uint32_t stride = gridDim.x * blockDim.x;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int d = 0; d < D; ++d) {
        unsigned long long above = 0ull, inf = 0ull;
        double mx = 0.0;
        for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < U; i += stride) {
            const unsigned long long len = (unsigned long long)((i + 1u < U ? useg[i + 1u] : T) - useg[i]);
            const double r = rhat[(uint64_t)d * U + i];
            if (r > threshold) above += len;
            if (r == __builtin_inf()) inf += len;
            else if (r > mx) mx = r;   // (not-a-number compares false: it is neither counted nor a maximum)
        }
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
            above += __shfl_xor(above, m);
            inf += __shfl_xor(inf, m);
            const double o = __shfl_xor(mx, m);
            mx = (o > mx) ? o : mx;
        }
        if (lane == 0) { sh_above[wave] = above; sh_inf[wave] = inf; sh_max[wave] = mx; }
        __syncthreads();
        if (threadIdx.x == 0) {
            double best = sh_max[0];
            for (int k = 1; k < 4; ++k) best = (sh_max[k] > best) ? sh_max[k] : best;
            const uint64_t o = (uint64_t)blockIdx.x * D + d;
            part_cnt[o * 2u] = sh_above[0] + sh_above[1] + sh_above[2] + sh_above[3];
            part_cnt[o * 2u + 1u] = sh_inf[0] + sh_inf[1] + sh_inf[2] + sh_inf[3];
            part_max[o] = best;
        }
        __syncthreads();
    }
}

#endif

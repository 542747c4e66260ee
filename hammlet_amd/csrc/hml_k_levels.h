// Posterior mean and spread of the emission LEVEL per position (no counterpart in the reference).
// The level of a recorded sweep at position t, dimension d, is mu[map[q_t][d]] under the theta that is current AFTER
// that sweep's parameter update.  Its sum and the sum of its squares over the recorded sweeps are label-invariant: they
// add over sweeps and over chains without any relabelling.  Device form, like hml_b_record: a difference array touched
// only where a run of equal states starts (rows 2 d = level, 2 d + 1 = level squared, T + 1 doubles each), and a boundary
// bitmap of the levels' own.  Read-out never walks the T cells: the bitmap is compacted into segment starts
// (hml_k_marg_count / hml_k_marg_scatter), the cells at the starts are gathered (hml_k_rec_gather) and scanned over the
// fixed tree of hml_k_scan.h, in double.
#ifndef HML_K_LEVELS_H
#define HML_K_LEVELS_H

#include "hml_math.h"
#include "hml_state.h"

// K11 levels_accumulate - one thread per block; launched AFTER the sweep's parameter kernel.
// Cell t of a row belongs to the one block that starts at t (plain read-modify-writes, the argument of hml_b_record), and a
// cell receives at most one term per sweep, in sweep order: the sums do not depend on the launch geometry.
HML_KERNEL __launch_bounds__(256) void hml_k_levels_record(const int16_t* __restrict__ q, const uint32_t* __restrict__ starts,
                                                           hml_model* __restrict__ mdl, double* __restrict__ acc,
                                                           uint32_t* __restrict__ boundary) {
    if (mdl->halted != 0u) return;   // (hml_state.h: the sweep did not happen; it is counted when it runs again)
    const uint32_t B = mdl->B;
    const uint64_t T1 = (uint64_t)mdl->T + 1u;
    const int D = mdl->D;
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t b = blockIdx.x * blockDim.x + threadIdx.x; b < B; b += stride) {
        const int st = q[b];
        const int prev = (b == 0) ? -1 : (int)q[b - 1];
        if (st != prev) {
            const uint32_t t = starts[b];
            for (int d = 0; d < D; ++d) {
                const double mn = (double)mdl->mu[mdl->map[st][d]];
                const double mp = (prev >= 0) ? (double)mdl->mu[mdl->map[prev][d]] : 0.0;
                acc[(uint64_t)(2 * d) * T1 + t] += mn - mp;
                acc[(uint64_t)(2 * d + 1) * T1 + t] += mn * mn - mp * mp;   // (squares of floats are exact in double)
            }
            atomicOr(&boundary[t >> 5], 1u << (t & 31u));
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&mdl->n_levels_recorded, 1ull);
}

// mean and standard deviation of the level per segment, as floats: ms[(2 d) * M + i] = S1 / N, ms[(2 d + 1) * M + i] =
// sqrt(max(0, S2 / N - (S1 / N)^2)), both in double before the one rounding to float (N = 0: not a number)
HML_KERNEL __launch_bounds__(256) void hml_k_levels_mean_sd(const double* __restrict__ g, uint32_t M, int D,
                                                            unsigned long long n_recorded, float* __restrict__ ms) {
    const uint32_t stride = gridDim.x * blockDim.x;
    const double N = (double)n_recorded;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < M; i += stride) {
        for (int d = 0; d < D; ++d) {
            float mean = __builtin_nanf(""), sd = __builtin_nanf("");
            if (n_recorded != 0ull) {
                const double m = g[(uint64_t)(2 * d) * M + i] / N;
                const double var = g[(uint64_t)(2 * d + 1) * M + i] / N - m * m;
                mean = (float)m;
                sd = (float)HML_SQRT(var > 0.0 ? var : 0.0);
            }
            ms[(uint64_t)(2 * d) * M + i] = mean;
            ms[(uint64_t)(2 * d + 1) * M + i] = sd;
        }
    }
}

// dense expansion, segment by segment: out[r][t] = ms[r][segment of t] for the 2 D rows.  A wavefront takes 64 consecutive
// positions; each lane finds its segment among the M sorted starts (seg_start[0] = 0).
HML_KERNEL __launch_bounds__(256) void hml_k_levels_expand(const float* __restrict__ ms, const uint32_t* __restrict__ seg_start,
                                                           uint32_t M, uint32_t T, int rows, float* __restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < T; t += stride) {
        uint32_t lo = 0u, hi = M;   // the last i with seg_start[i] <= t
        while (hi - lo > 1u) {
            const uint32_t mid = lo + (hi - lo) / 2u;
            if (seg_start[mid] <= (uint32_t)t) lo = mid; else hi = mid;
        }
        for (int r = 0; r < rows; ++r) out[(uint64_t)r * T + t] = ms[(uint64_t)r * M + lo];
    }
}

#endif

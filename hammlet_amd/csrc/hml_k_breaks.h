// Breakpoint posteriors per position and the consensus segmentation (no counterpart in the reference; DESIGN.md 3c'').
// A recorded sweep has a BREAKPOINT at position t (0 < t < T) iff block b > 0 starts at t and q[b] != q[b - 1]; position 0
// is never one.  C[t] counts the recorded sweeps with a breakpoint at t, N the sweeps recorded while the recording was on.
// Like the emission level the indicator is label-invariant: it adds over sweeps and chains without relabelling; unlike it
// everything here is an integer, so every read-out is exact.  Device form, like hml_k_levels_record: uint32 [T + 1], touched
// only where a run of equal states starts, and a boundary bitmap of the breaks' own.  Read-out never walks the T cells: the
// bitmap is compacted into the M break positions (hml_k_marg_count / hml_k_marg_scatter; entry 0 of that list is the
// position 0 those kernels always emit and is dropped), the counts are gathered (hml_k_rec_gather, one row) and scanned
// (hml_k_scan.h: 32-bit counts into exclusive 64-bit sums pre[i] = sum of v[j] over j < i, pre[M] = the total).
#ifndef HML_K_BREAKS_H
#define HML_K_BREAKS_H

#include "hml_state.h"

// K12 breaks_accumulate - one thread per block.  Cell t belongs to the one block that starts at t (plain read-modify-write,
// the argument of hml_b_record), and a cell receives at most one increment per sweep.  Does not read theta: it may run
// before or behind the sweep's parameter kernel.
HML_KERNEL __launch_bounds__(256) void hml_k_breaks_record(const int16_t* __restrict__ q, const uint32_t* __restrict__ starts,
                                                           hml_model* __restrict__ mdl, uint32_t* __restrict__ cnt,
                                                           uint32_t* __restrict__ boundary) {
    if (mdl->halted != 0u) return;   // (hml_state.h: the sweep did not happen; it is counted when it runs again)
    const uint32_t B = mdl->B;
    const uint32_t T = mdl->T;
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t b = blockIdx.x * blockDim.x + threadIdx.x; b < B; b += stride) {
        if (b == 0u || q[b] == q[b - 1]) continue;
        const uint32_t t = starts[b];
        if (t == 0u || t >= T) continue;   // (never: block b > 0 starts inside (0, T))
        cnt[t] += 1u;
        atomicOr(&boundary[t >> 5], 1u << (t & 31u));
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&mdl->n_breaks_recorded, 1ull);
}

// the first i in [0, M] with pos[i] >= key (key may exceed every position: M)
__device__ __forceinline__ uint32_t hml_breaks_lower(const uint32_t* __restrict__ pos, uint32_t M, uint64_t key) {
    uint32_t lo = 0u, hi = M;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if ((uint64_t)pos[mid] < key) lo = mid + 1u; else hi = mid;
    }
    return lo;
}

// hml_breaks_dense_device: out[t] = (sum of C[u] over |u - t| <= window) / N - the sum exact in 64-bit integers, the
// quotient in double, one rounding to float; not a number when N = 0
HML_KERNEL __launch_bounds__(256) void hml_k_breaks_dense(const uint32_t* __restrict__ pos, const unsigned long long* __restrict__ pre,
                                                          uint32_t M, uint32_t T, uint32_t window, unsigned long long n_recorded,
                                                          float* __restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const double N = (double)n_recorded;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < T; t += stride) {
        float v = __builtin_nanf("");
        if (n_recorded != 0ull) {
            const uint32_t a = hml_breaks_lower(pos, M, t > window ? t - window : 0ull);
            const uint32_t b = hml_breaks_lower(pos, M, t + (uint64_t)window + 1ull);
            v = (float)((double)(pre[b] - pre[a]) / N);
        }
        out[t] = v;
    }
}

// hml_breaks_consensus, candidate by candidate: mass[i] = sum of C_j over |t_j - t_i| <= window; selected[i] = 1 iff
// mass[i] >= min_count and no other candidate j of the window has C_j > C_i, or C_j == C_i with t_j < t_i (whether j is
// selected itself plays no part).  Two binary searches and a scan of the window; nothing is shared between candidates.
HML_KERNEL __launch_bounds__(256) void hml_k_breaks_select(const uint32_t* __restrict__ pos, const uint32_t* __restrict__ cnt,
                                                           const unsigned long long* __restrict__ pre, uint32_t M, uint32_t window,
                                                           unsigned long long min_count, unsigned long long* __restrict__ mass,
                                                           uint32_t* __restrict__ selected) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < M; i += stride) {
        const uint64_t t = pos[i];
        const uint32_t ci = cnt[i];
        const uint32_t a = hml_breaks_lower(pos, M, t > window ? t - window : 0ull);
        const uint32_t b = hml_breaks_lower(pos, M, t + (uint64_t)window + 1ull);
        const unsigned long long m = pre[b] - pre[a];
        bool keep = m >= min_count;
        for (uint32_t j = a; j < b && keep; ++j) {
            if (j == i) continue;
            const uint32_t cj = cnt[j];
            if (cj > ci || (cj == ci && j < i)) keep = false;
        }
        mass[i] = m;
        selected[i] = keep ? 1u : 0u;
    }
}

// the selected candidates, ascending, at the places the exclusive sums of `selected` give them
HML_KERNEL __launch_bounds__(256) void hml_k_breaks_compact(const uint32_t* __restrict__ pos, const uint32_t* __restrict__ cnt,
                                                            const unsigned long long* __restrict__ mass, const uint32_t* __restrict__ selected,
                                                            const unsigned long long* __restrict__ where, uint32_t M,
                                                            uint32_t* __restrict__ out_pos, unsigned long long* __restrict__ out_mass,
                                                            uint32_t* __restrict__ out_peak) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < M; i += stride) {
        if (!selected[i]) continue;
        const unsigned long long k = where[i];
        out_pos[k] = pos[i];
        out_mass[k] = mass[i];
        out_peak[k] = cnt[i];
    }
}

// ---- hml_levels_on_segments (the levels' accumulators, hml_k_levels.h, summed over caller-given segments) ----
// w[r][i] = len_i * v[r][i]: the sum of row r over the positions of fine segment i (v: the inclusive sums of the gathered
// cells = the row's value on the segment; seg_start[M] sorted, seg_start[0] = 0)
HML_KERNEL __launch_bounds__(256) void hml_k_levels_weigh(const double* __restrict__ v, const uint32_t* __restrict__ seg_start,
                                                          uint32_t M, uint32_t T, int rows, double* __restrict__ w) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < M; i += stride) {
        const double len = (double)((i + 1u < M ? seg_start[i + 1u] : T) - seg_start[i]);
        for (int r = 0; r < rows; ++r) w[(uint64_t)r * M + i] = len * v[(uint64_t)r * M + i];
    }
}

// F(x) = sum of the row over the positions below x: the prefix sum of w over the fine segments that end at or before x,
// plus (x - start) * value of the fine segment that holds x
__device__ __forceinline__ double hml_levels_below(const double* __restrict__ v, const double* __restrict__ pw,
                                                   const uint32_t* __restrict__ seg_start, uint32_t M, uint32_t T, uint32_t x) {
    if (x >= T) return pw[M - 1u];
    uint32_t lo = 0u, hi = M;   // the last i with seg_start[i] <= x
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (seg_start[mid] <= x) lo = mid; else hi = mid;
    }
    const double part = (double)(x - seg_start[lo]) * v[lo];
    return lo > 0u ? pw[lo - 1u] + part : part;
}

// out[r][k] = F(end of segment k) - F(its start) for the n_cuts + 1 segments between 0, the cuts and T
HML_KERNEL __launch_bounds__(256) void hml_k_levels_on_segments(const double* __restrict__ v, const double* __restrict__ pw,
                                                                const uint32_t* __restrict__ seg_start, uint32_t M, uint32_t T,
                                                                int rows, const uint32_t* __restrict__ cuts, uint32_t n_cuts,
                                                                double* __restrict__ out) {
    const uint32_t n_seg = n_cuts + 1u;
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < n_seg; k += stride) {
        const uint32_t a = (k == 0u) ? 0u : cuts[k - 1u];
        const uint32_t b = (k == n_cuts) ? T : cuts[k];
        for (int r = 0; r < rows; ++r) {
            const double* vr = v + (uint64_t)r * M;
            const double* pr = pw + (uint64_t)r * M;
            out[(uint64_t)r * n_seg + k] = hml_levels_below(vr, pr, seg_start, M, T, b) - hml_levels_below(vr, pr, seg_start, M, T, a);
        }
    }
}

#endif

// Posterior of the emission level in caller-given BANDS per position (no counterpart in the reference; DESIGN.md 3c''').
// The caller gives n ascending edges; band(mu) = the number of edges e with e <= mu (compared in float; not a number: band 0),
// so there are n + 1 bands per data dimension and D (n + 1) columns, column d (n + 1) + b.  The chain counts, per position
// and column, the recorded sweeps whose level - hml_k_levels.h's: mu[map[q_t][d]] under the theta that is current after the
// sweep's parameter update - fell into the band.  The label-free counterpart of the state marginals: it adds over sweeps and
// chains without relabelling, and everything is an integer, so every read-out is exact.  Device form, the marginals': int32
// difference arrays [columns][T + 1] and a boundary bitmap of the bands' own, touched only where the BAND VECTOR changes -
// adjacent runs of different states in the same bands leave no cell and no bit.  Read-out never walks the T cells (but for the
// dense form): hml_k_marg_count / _scatter / _gather compact the bitmap and gather the cells, hml_k_seg_partial and
// hml_k_scan_chunks scan them, hml_k_seg_run_count / _run_scatter merge the calls into runs.
#ifndef HML_K_BANDS_H
#define HML_K_BANDS_H

#include "hml_state.h"

#define HML_MAX_BAND_EDGES 31

// the edges, a kernel argument by value
struct hml_band_edges {
    int32_t n;
    float e[HML_MAX_BAND_EDGES];
};

HML_HD int hml_band_of(const hml_band_edges& ed, float mu) {
    int b = 0;
    for (int j = 0; j < ed.n; ++j) b += (ed.e[j] <= mu) ? 1 : 0;   // (false for every edge when mu is not a number)
    return b;
}

// K13 bands_accumulate - one thread per block; launched AFTER the sweep's parameter kernel, like hml_k_levels_record.  Every
// workgroup first writes the band of each of the P emission parameters into LDS; a block then costs look-ups through the
// state mapping.  Cell t of a row belongs to the one block that starts at t (plain read-modify-writes, the argument of
// hml_b_record), and a cell receives at most one term per sweep.
HML_KERNEL __launch_bounds__(256) void hml_k_bands_record(const int16_t* __restrict__ q, const uint32_t* __restrict__ starts,
                                                          hml_model* __restrict__ mdl, const hml_band_edges edges,
                                                          int32_t* __restrict__ acc, uint32_t* __restrict__ boundary) {
    if (mdl->halted != 0u) return;   // (hml_state.h: the sweep did not happen; it is counted when it runs again)
    __shared__ uint8_t band_of[HML_CAP_K];
    const int P = mdl->P < HML_CAP_K ? mdl->P : HML_CAP_K;
    if ((int)threadIdx.x < P) band_of[threadIdx.x] = (uint8_t)hml_band_of(edges, mdl->mu[threadIdx.x]);
    __syncthreads();
    const uint32_t B = mdl->B;
    const uint32_t T = mdl->T;
    const uint64_t T1 = (uint64_t)T + 1u;
    const int D = mdl->D;
    const int nb = edges.n + 1;
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t b = blockIdx.x * blockDim.x + threadIdx.x; b < B; b += stride) {
        const int st = q[b];
        const int prev = (b == 0) ? -1 : (int)q[b - 1];
        if (st == prev) continue;
        int bn[HML_MAX_D], bp[HML_MAX_D];
        bool changed = false;
#pragma unroll
        for (int d = 0; d < HML_MAX_D; ++d) {
            if (d < D) {
                bn[d] = band_of[mdl->map[st][d]];
                bp[d] = (prev >= 0) ? (int)band_of[mdl->map[prev][d]] : -1;
                changed = changed || bn[d] != bp[d];
            }
        }
        if (!changed) continue;   // (another state in the same bands: no cell, no bit)
        const uint32_t t = starts[b];
        if (t >= T) continue;   // (never: a block starts inside [0, T))
#pragma unroll
        for (int d = 0; d < HML_MAX_D; ++d) {
            if (d < D && bn[d] != bp[d]) {
                acc[(uint64_t)(d * nb + bn[d]) * T1 + t] += 1;
                if (bp[d] >= 0) acc[(uint64_t)(d * nb + bp[d]) * T1 + t] -= 1;
            }
        }
        atomicOr(&boundary[t >> 5], 1u << (t & 31u));
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&mdl->n_bands_recorded, 1ull);
}

// hml_bands_dense_device, cumulative form: in place over out[columns][T], row b of a dimension becomes the sum of its rows
// b, b + 1, ... (the sweeps whose level lay in band b or above; row 0: all of them)
HML_KERNEL __launch_bounds__(256) void hml_k_bands_cumulate(int32_t* __restrict__ out, uint32_t T, int D, int nb) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < T; t += stride) {
        for (int d = 0; d < D; ++d) {
            int32_t run = 0;
            for (int b = nb - 1; b >= 0; --b) {
                const uint64_t at = (uint64_t)(d * nb + b) * T + t;
                run += out[at];
                out[at] = run;
            }
        }
    }
}

// hml_bands_call: the band called for every band segment and dimension, from the count differences at the segment starts
// g[M][columns] (hml_k_marg_gather) and the exclusive sums of their chunks of 256 segments (hml_k_seg_partial, then
// hml_k_scan_chunks).  rank 0: the band with the largest count - first maximum, strict `>` from count 0, hml_k_seg_argmax's
// rule; rank >= 1: the smallest band whose cumulative count over the bands up to it reaches `rank` (the last band if none does).
// The D calls of a segment are packed into one key, sum over d of call_d nb^d - below 2^16 because D nb <= HML_CAP_K and
// D <= HML_MAX_D - so that hml_k_seg_run_count / hml_k_seg_run_scatter merge equal neighbours; keys compare as bit patterns.
HML_KERNEL __launch_bounds__(256) void hml_k_bands_pick(const int32_t* __restrict__ g, uint32_t M, int D, int nb,
                                                        const int32_t* __restrict__ chunk_base, uint32_t n_chunks,
                                                        unsigned long long rank, int16_t* __restrict__ seg_key) {
    __shared__ int32_t wsum[4][HML_CAP_K];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ncol = D * nb;
    for (int s = 0; s < ncol; ++s) {
        int32_t v = i < M ? g[(uint64_t)i * ncol + s] : 0;
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m);
        if (lane == 0) wsum[wave][s] = v;
    }
    __syncthreads();
    uint32_t key = 0u, scale = 1u;
    for (int d = 0; d < D; ++d) {
        int best = 0;
        int32_t best_count = 0;
        long long cum = 0;
        bool found = false;
        for (int b = 0; b < nb; ++b) {
            const int s = d * nb + b;
            int32_t v = i < M ? g[(uint64_t)i * ncol + s] : 0;
#pragma unroll
            for (int k = 1; k < 64; k <<= 1) {
                const int32_t o = __shfl_up(v, k);
                if (lane >= k) v += o;
            }
            int32_t c = chunk_base[(uint64_t)s * n_chunks + blockIdx.x] + v;
            for (int w2 = 0; w2 < wave; ++w2) c += wsum[w2][s];
            if (rank == 0ull) {
                if (c > best_count) { best_count = c; best = b; }
            } else {
                cum += c;
                if (!found && cum >= (long long)rank) { found = true; best = b; }
            }
        }
        if (rank != 0ull && !found) best = nb - 1;
        key += (uint32_t)best * scale;
        scale *= (uint32_t)nb;
    }
    if (i < M) seg_key[i] = (int16_t)(uint16_t)key;
}

#endif

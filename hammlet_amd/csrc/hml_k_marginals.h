// Finalisation of the state marginals: boundary compaction, per-segment gathers, dense expansion - and what the other
// per-position recordings (levels, breaks, bands: hml_recorder, hml_ctx.hpp) share with them: the compaction of a boundary
// bitmap, the gather of a recording's cells at the starts and the merge of one chain's recording into another's.
#ifndef HML_K_MARGINALS_H
#define HML_K_MARGINALS_H

#include "hml_state.h"

// count boundary bits per span of 4096 positions (128 words); position 0 always counts
HML_KERNEL __launch_bounds__(256) void hml_k_marg_count(const uint32_t* __restrict__ boundary, uint32_t T,
                                                        uint32_t* __restrict__ span_count) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t span = blockIdx.x * 4u + (uint32_t)wave;
    const uint64_t base = (uint64_t)span * HML_SPAN;
    if (base >= T) return;
    uint32_t cnt = 0;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const uint64_t word = base / 32u + (uint64_t)lane + 64u * k;
        const uint64_t t0 = word * 32u;
        uint32_t bits = (t0 < T) ? boundary[word] : 0u;
        if (t0 < T && t0 + 32u > T) bits &= (1u << (T - t0)) - 1u;
        if (word == 0) bits |= 1u;
        cnt += __popc(bits);
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) cnt += __shfl_xor(cnt, m);
    if (lane == 0) span_count[span] = cnt;
}

// write the boundary positions of each span, in order, at seg_start[span_offset + ...]
HML_KERNEL __launch_bounds__(256) void hml_k_marg_scatter(const uint32_t* __restrict__ boundary, uint32_t T,
                                                          const uint32_t* __restrict__ span_offset,
                                                          uint32_t* __restrict__ seg_start) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t span = blockIdx.x * 4u + (uint32_t)wave;
    const uint64_t base = (uint64_t)span * HML_SPAN;
    if (base >= T) return;
    uint32_t run = span_offset[span];
    for (int k = 0; k < 2; ++k) {
        const uint64_t word = base / 32u + (uint64_t)lane + 64u * k;
        const uint64_t t0 = word * 32u;
        uint32_t bits = (t0 < T) ? boundary[word] : 0u;
        if (t0 < T && t0 + 32u > T) bits &= (1u << (T - t0)) - 1u;
        if (word == 0) bits |= 1u;
        const uint32_t c = __popc(bits);
        // exclusive prefix of c across the wavefront
        uint32_t incl = c;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t o = __shfl_up(incl, d);
            if (lane >= d) incl += o;
        }
        uint32_t pos = run + incl - c;
        while (bits) {
            const int bit = __ffs(bits) - 1;
            bits &= bits - 1u;
            seg_start[pos++] = (uint32_t)(t0 + (uint64_t)bit);
        }
        run += __shfl(incl, 63);
    }
}

// gather diff[s][seg_start[i]] for all states: out[i*K + s]
HML_KERNEL __launch_bounds__(256) void hml_k_marg_gather(const int32_t* __restrict__ diff, uint32_t T, int K,
                                                         const uint32_t* __restrict__ seg_start, uint32_t M,
                                                         int32_t* __restrict__ out) {
    const uint64_t T1 = (uint64_t)T + 1u;
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < M; i += stride) {
        const uint32_t t = seg_start[i];
        for (int s = 0; s < K; ++s) out[(uint64_t)i * K + s] = diff[(uint64_t)s * T1 + t];
    }
}

// a recording's cells at the listed positions, row by row: out[r * M + i] = acc[r][pos[i]]
template <typename E>
__global__ __launch_bounds__(256) void hml_k_rec_gather(const E* __restrict__ acc, uint32_t T, int rows,
                                                        const uint32_t* __restrict__ pos, uint32_t M, E* __restrict__ out) {
    const uint64_t T1 = (uint64_t)T + 1u;
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < M; i += stride) {
        const uint32_t t = pos[i];
        for (int r = 0; r < rows; ++r) out[(uint64_t)r * M + i] = acc[(uint64_t)r * T1 + t];
    }
}

// hml_levels_merge / hml_breaks_merge / hml_bands_merge: the source's cells at the source's M listed positions into the
// destination (same T, same rows), its boundary bits, its count of recorded sweeps (src_n, dst_n: the two counters inside
// the chains' hml_model).  The positions are distinct: plain read-modify-writes.
template <typename E>
__global__ __launch_bounds__(256) void hml_k_rec_merge(const E* __restrict__ src, const uint32_t* __restrict__ pos, uint32_t M,
                                                       uint32_t T, int rows, const unsigned long long* __restrict__ src_n,
                                                       E* __restrict__ dst, uint32_t* __restrict__ dst_boundary,
                                                       unsigned long long* __restrict__ dst_n) {
    const uint64_t T1 = (uint64_t)T + 1u;
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < M; i += stride) {
        const uint32_t t = pos[i];
        for (int r = 0; r < rows; ++r) dst[(uint64_t)r * T1 + t] += src[(uint64_t)r * T1 + t];
        atomicOr(&dst_boundary[t >> 5], 1u << (t & 31u));
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(dst_n, *src_n);
}

// ---- dense expansion: counts[s][t] = prefix sum over t of diff[s][t]; row K = boundary indicator ----
// three-phase scan over chunks of 4096 positions per state; the middle phase is hml_k_scan_chunks<int32_t> (hml_k_scan.h)
HML_KERNEL __launch_bounds__(256) void hml_k_dense_partial(const int32_t* __restrict__ diff, uint32_t T, int K,
                                                           int32_t* __restrict__ chunk_sum, uint32_t n_chunks) {
    __shared__ int32_t red[4];
    const int s = blockIdx.y;
    const uint32_t chunk = blockIdx.x;
    const uint64_t T1 = (uint64_t)T + 1u;
    const uint64_t base = (uint64_t)chunk * HML_SPAN;
    int32_t acc = 0;
    for (int k = 0; k < 16; ++k) {
        const uint64_t t = base + (uint64_t)k * 256u + threadIdx.x;
        if (t < T) acc += diff[(uint64_t)s * T1 + t];
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) acc += __shfl_xor(acc, m);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) chunk_sum[(uint64_t)s * n_chunks + chunk] = red[0] + red[1] + red[2] + red[3];
}

HML_KERNEL __launch_bounds__(256) void hml_k_dense_final(const int32_t* __restrict__ diff, uint32_t T, int K,
                                                         const int32_t* __restrict__ chunk_sum, uint32_t n_chunks,
                                                         const int32_t* __restrict__ perm, int32_t* __restrict__ out) {
    __shared__ int32_t wsum[4];
    const int snew = blockIdx.y;
    const int s = perm ? perm[snew] : snew;
    const uint32_t chunk = blockIdx.x;
    const uint64_t T1 = (uint64_t)T + 1u;
    const uint64_t base = (uint64_t)chunk * HML_SPAN;
    int32_t run = chunk_sum[(uint64_t)s * n_chunks + chunk];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int k = 0; k < 16; ++k) {
        const uint64_t t = base + (uint64_t)k * 256u + threadIdx.x;
        const int32_t v = (t < T) ? diff[(uint64_t)s * T1 + t] : 0;
        int32_t incl = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int32_t o = __shfl_up(incl, d);
            if (lane >= d) incl += o;
        }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        int32_t before = 0;
        for (int w2 = 0; w2 < wave; ++w2) before += wsum[w2];
        const int32_t total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        if (t < T) out[(uint64_t)snew * T + t] = run + before + incl;
        run += total;
        __syncthreads();
    }
}

HML_KERNEL __launch_bounds__(256) void hml_k_dense_boundary(const uint32_t* __restrict__ boundary, uint32_t T,
                                                            int32_t* __restrict__ out_row) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < T; t += stride)
        out_row[t] = (t == 0) ? 1 : (int32_t)((boundary[t >> 5] >> (t & 31u)) & 1u);
}

#endif

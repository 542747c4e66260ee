// The one prefix sum of the read-outs: a three-phase scan over a tree of FIXED shape, for every number type they use.
//   double -> double, inclusive, in place, one row per blockIdx.y   the levels' segment sums (hml_k_levels.h)
//   uint32 -> uint64, exclusive, the total in [M]                   the breaks' counts and selections (hml_k_breaks.h)
//   int32, the chunk-total phase alone                               behind hml_k_dense_partial / hml_k_seg_partial
// The tree over the M entries of a row: chunks of HML_SCAN_CHUNK entries; inside a chunk four consecutive entries per
// thread, added one after the other from zero, then 8 doubling steps over the 256 threads' sums, and thread i > 0 puts the
// sum of thread i - 1 in front of its four; the chunk totals in 1024 pieces of ceil(chunks / 1024), each added up from zero,
// 10 doubling steps over the pieces, and piece i > 0 runs on from the sum of piece i - 1; last, `base + v` per entry.  Which
// additions happen, and in which order, depends on M alone - not on the grid, which only decides which workgroup takes which
// chunk.  The levels' sums are doubles and are promised bit for bit (tests/levels_util.py restates this tree), so two details
// that no integer could tell apart are part of the tree:
//   - a doubling step adds only where there is a partner (`if (tid >= d)`): adding a zero instead would turn -0.0 into +0.0;
//   - a piece starts from part[tid - 1], not from part[tid] - sum: in double these are not the same number.
#ifndef HML_K_SCAN_H
#define HML_K_SCAN_H

#include "hml_state.h"

#define HML_SCAN_CHUNK 1024

// inclusive sums of one chunk's entries, relative to the chunk's start (the calling workgroup's 256 threads; `sh`: 256 sums)
template <typename In, typename Acc>
__device__ __forceinline__ void hml_scan_chunk(const In* row, uint32_t M, uint32_t chunk, Acc* sh, Acc v[4]) {
    const uint32_t tid = threadIdx.x;
    const uint64_t i0 = (uint64_t)chunk * HML_SCAN_CHUNK + 4u * tid;
    Acc run = Acc(0);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (i0 + k < M) run += row[i0 + k];
        v[k] = run;
    }
    sh[tid] = run;
    __syncthreads();
    for (uint32_t d = 1; d < 256u; d <<= 1) {
        const Acc o = (tid >= d) ? sh[tid - d] : Acc(0);
        __syncthreads();
        if (tid >= d) sh[tid] += o;
        __syncthreads();
    }
    if (tid > 0) {
        const Acc before = sh[tid - 1];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = before + v[k];
    }
}

// grid (any x, rows): chunk totals, chunk_sum[row][n_chunks]
template <typename In, typename Acc>
__global__ __launch_bounds__(256) void hml_k_scan_partial(const In* __restrict__ in, uint32_t M, uint32_t n_chunks,
                                                          Acc* __restrict__ chunk_sum) {
    __shared__ Acc sh[256];
    const In* row = in + (uint64_t)blockIdx.y * M;
    for (uint32_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        Acc v[4];
        hml_scan_chunk(row, M, chunk, sh, v);
        if (threadIdx.x == 255u) chunk_sum[(uint64_t)blockIdx.y * n_chunks + chunk] = v[3];
        __syncthreads();
    }
}

// grid (rows): exclusive sums of a row's n_chunks totals, in place
template <typename Acc>
__global__ __launch_bounds__(1024) void hml_k_scan_chunks(Acc* __restrict__ chunk_sum, uint32_t n_chunks) {
    __shared__ Acc part[1024];
    Acc* cs = chunk_sum + (uint64_t)blockIdx.x * n_chunks;
    const uint32_t tid = threadIdx.x;
    const uint32_t per = (n_chunks + 1023u) / 1024u;
    const uint32_t a = (uint64_t)tid * per < n_chunks ? tid * per : n_chunks;
    const uint32_t b = (a + per < n_chunks) ? a + per : n_chunks;
    Acc sum = Acc(0);
    for (uint32_t i = a; i < b; ++i) sum += cs[i];
    part[tid] = sum;
    __syncthreads();
    for (uint32_t d = 1; d < 1024u; d <<= 1) {
        const Acc o = (tid >= d) ? part[tid - d] : Acc(0);
        __syncthreads();
        if (tid >= d) part[tid] += o;
        __syncthreads();
    }
    Acc run = (tid > 0) ? part[tid - 1] : Acc(0);
    for (uint32_t i = a; i < b; ++i) { const Acc x = cs[i]; cs[i] = run; run += x; }
}

// grid (any x, rows).  Inclusive: out[row][M], out[i] = the sum up to and including entry i (`out` may be `in`: a thread
// writes the four places it read).  Exclusive: out[row][M + 1], out[i] = the sum below entry i, out[M] = the total.
template <typename In, typename Acc, bool Exclusive>
__global__ __launch_bounds__(256) void hml_k_scan_final(const In* in, uint32_t M, uint32_t n_chunks,
                                                        const Acc* __restrict__ chunk_sum, Acc* out) {
    __shared__ Acc sh[256];
    const uint32_t shift = Exclusive ? 1u : 0u;
    const In* row = in + (uint64_t)blockIdx.y * M;
    Acc* orow = out + (uint64_t)blockIdx.y * ((uint64_t)M + shift);
    if (Exclusive && blockIdx.x == 0 && threadIdx.x == 0) orow[0] = Acc(0);
    for (uint32_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        Acc v[4];
        hml_scan_chunk(row, M, chunk, sh, v);
        const Acc base = chunk_sum[(uint64_t)blockIdx.y * n_chunks + chunk];
        const uint64_t i0 = (uint64_t)chunk * HML_SCAN_CHUNK + 4u * threadIdx.x;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (i0 + k < M) orow[i0 + k + shift] = base + v[k];
        __syncthreads();
    }
}

#endif

// The sparse payload of a recording (include/hml.h, hml_recording_export / hml_recording_merge_payload): what one chain's
// emission levels, breakpoint counts or level bands are once the T + 1 cells per row that no sweep touched are left out -
// a header, the bands' edges, the M positions with a cell and the rows' RAW cells there (the differences the record kernels
// accumulate, not their prefix sums: adding them into another recorder is the addition hml_k_rec_merge performs, cell by cell).
// One contiguous little-endian buffer, the same for the three kinds:
//     uint64 header[8]   magic, kind, T, rows, M, N, bytes per cell, n_band_edges
//     float  edges[32]   the bands' edges followed by zeros (all zero for the other kinds)
//     uint32 pos[M]      strictly ascending, < T (breaks: > 0); zero bytes up to a multiple of 8
//     E      cells[rows][M]   cells[r * M + i] = acc[r][pos[i]]  (hml_k_rec_gather writes them in place)
// Nothing here runs inside a sweep.
#ifndef HML_K_REC_PAYLOAD_H
#define HML_K_REC_PAYLOAD_H

#include "hml_k_bands.h"
#include "hml_state.h"

#define HML_RECPAY_MAGIC 0x00314345524C4D48ull   // the bytes "HMLREC1\0"
#define HML_RECPAY_HEADER_WORDS 8
#define HML_RECPAY_EDGE_SLOTS 32
#define HML_RECPAY_FIXED_BYTES (HML_RECPAY_HEADER_WORDS * 8 + HML_RECPAY_EDGE_SLOTS * 4)   // 192

// what the position check found, one bit per fault (hml_k_recpay_check)
#define HML_RECPAY_BAD_ORDER 1u   // pos[i] <= pos[i - 1]
#define HML_RECPAY_BAD_RANGE 2u   // pos[i] >= T
#define HML_RECPAY_BAD_ZERO 4u    // pos[i] < the kind's smallest position (breaks: position 0 is never a breakpoint)

// header and edges of a payload of M positions: N is the recorder's count of recorded sweeps, read from the counter inside
// the chain's hml_model; the odd position's padding word is zeroed here as well.  One wavefront.
HML_KERNEL __launch_bounds__(64) void hml_k_recpay_header(unsigned long long* __restrict__ out, unsigned long long kind, unsigned long long T,
                                                          unsigned long long rows, unsigned long long M,
                                                          const unsigned long long* __restrict__ n_recorded, unsigned long long cell_bytes,
                                                          const hml_band_edges ed) {
    const int lane = threadIdx.x;
    if (lane == 0) {
        out[0] = HML_RECPAY_MAGIC; out[1] = kind; out[2] = T; out[3] = rows;
        out[4] = M; out[5] = *n_recorded; out[6] = cell_bytes; out[7] = (unsigned long long)ed.n;
    }
    float* const edges = reinterpret_cast<float*>(out + HML_RECPAY_HEADER_WORDS);
    if (lane < HML_RECPAY_EDGE_SLOTS) edges[lane] = (lane < ed.n && lane < HML_MAX_BAND_EDGES) ? ed.e[lane] : 0.0f;
    if (lane == 63 && (M & 1ull)) reinterpret_cast<uint32_t*>(out + HML_RECPAY_FIXED_BYTES / 8)[M] = 0u;
}

// Are the M positions of a payload strictly ascending, below T and at least min_pos?  Each thread compares pos[i] with
// pos[i - 1]; the faults are OR-ed over the wavefront by shuffles, over the workgroup in shared memory, and a workgroup
// that found one reports it with a single atomic.  *flag was zeroed by the caller; nothing else is written.
HML_KERNEL __launch_bounds__(256) void hml_k_recpay_check(const uint32_t* __restrict__ pos, uint32_t M, uint32_t T, uint32_t min_pos,
                                                          uint32_t* __restrict__ flag) {
    __shared__ uint32_t wave_bad[4];
    uint32_t bad = 0u;
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < M; i += stride) {
        const uint32_t p = pos[i];
        if (p >= T) bad |= HML_RECPAY_BAD_RANGE;
        if (p < min_pos) bad |= HML_RECPAY_BAD_ZERO;
        if (i > 0u && pos[i - 1u] >= p) bad |= HML_RECPAY_BAD_ORDER;
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) bad |= __shfl_xor(bad, m);
    if ((threadIdx.x & 63) == 0) wave_bad[threadIdx.x >> 6] = bad;
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t all = wave_bad[0] | wave_bad[1] | wave_bad[2] | wave_bad[3];
        if (all) atomicOr(flag, all);
    }
}

// hml_recording_merge_payload: the payload's cells into the destination's recorder at the listed positions, its boundary
// bits, its count of recorded sweeps - the additions of hml_k_rec_merge with the source's cells read from the list.  One
// thread per position and a loop over the rows: the cell reads are coalesced along i; the positions were checked to be
// distinct and below T (hml_k_recpay_check), so the scattered read-modify-writes are plain.
template <typename E>
__global__ __launch_bounds__(256) void hml_k_rec_merge_list(const uint32_t* __restrict__ pos, const E* __restrict__ cells, uint32_t M,
                                                            uint32_t T, int rows, unsigned long long n_recorded, E* __restrict__ dst,
                                                            uint32_t* __restrict__ dst_boundary, unsigned long long* __restrict__ dst_n) {
    const uint64_t T1 = (uint64_t)T + 1u;
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < M; i += stride) {
        const uint32_t t = pos[i];
        for (int r = 0; r < rows; ++r) dst[(uint64_t)r * T1 + t] += cells[(uint64_t)r * M + i];
        atomicOr(&dst_boundary[t >> 5], 1u << (t & 31u));
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(dst_n, n_recorded);
}

#endif

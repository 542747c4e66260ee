// Joint posteriors over caller-given REGIONS, recorded per sweep (no counterpart in the reference; DESIGN.md 3c'''''').
// A region is a half-open range of positions [a, e).  A recorded sweep - its block starts, its states and the theta that is
// current after its parameter update, the pairing of hml_k_levels.h - gives per region
//   nb    the breakpoints strictly inside it: the blocks b in (blk(a), blk(e - 1)] with q[b] != q[b - 1];
//   same  per data dimension, whether every block of the region lies in one band of the region's own edges, and which;
//   m     per data dimension, the mean level of the region's positions, (1 / len) sum over blocks of overlap x level, in double.
// None of these follows from the per-position recordings: the positions of a region are correlated within a sweep.  The
// accumulators are a few words per region (hml_regions_acc below) and add over sweeps, chains and GPUs without relabelling.
//
// Three launches per recorded sweep, behind the parameter kernel, all of which read the block count from the model:
//   hml_k_regions_chunks      per chunk of HML_RG_CHUNK blocks: state changes, band changes per dimension, sum of length x level;
//   hml_k_regions_scan        exclusive sums of the chunk totals, one workgroup per row, over a tree that ceil(B / chunk) fixes;
//   hml_k_regions_accumulate  a wavefront per region: the two end blocks by a 64-ary search over the block starts, the two
//                             partial chunks by the lanes, the whole chunks in between from the sums.
// Which double additions happen, and in which order, depends on the sweep's (B, starts, q, theta) and the region alone - not
// on a grid, on the block capacity or on the sweep path that produced the blocks.
#ifndef HML_K_REGIONS_H
#define HML_K_REGIONS_H

#include "hml_k_bands.h"
#include "hml_state.h"

#define HML_RG_CHUNK 256u   // blocks per chunk: one workgroup of hml_k_regions_chunks, a block a thread
#define HML_RG_SHIFT 8

// the accumulators of n regions, views into one allocation (ncol = D (n_edges + 1), 0 without edges)
struct hml_regions_acc {
    unsigned long long* whole;        // [n]        sweeps without a breakpoint inside
    unsigned long long* breaks_sum;   // [n]        sum of nb
    unsigned long long* breaks_sq;    // [n]        sum of nb^2, saturating
    double* level_sum;                // [D][n]     sum of m_d
    double* level_sq;                 // [D][n]     sum of m_d^2
    unsigned long long* inband;       // [n][ncol]  sweeps with every block of the region in band j of dimension d
};

// the chunk totals and, after the scan, their exclusive sums: rows of `stride` entries
struct hml_regions_chunks {
    uint32_t* cnt;    // [1 + D][stride]: row 0 state changes, row 1 + d band changes of dimension d
    double* lev;      // [D][stride]: sum over the chunk's blocks of length x level
    uint32_t stride;
};

HML_HD unsigned long long hml_sat_add_u64(unsigned long long a, unsigned long long b) {
    const unsigned long long s = a + b;
    return s < a ? ~0ull : s;
}

// The kernels below are compiled into the ONE object that launches them (hml_readout.hip defines HML_REGIONS_KERNELS): the
// device pass emits every kernel it sees, launched from that object or not, and the code objects of the sweeps and of the
// core are to hold exactly what they held before.
#if defined(HML_REGIONS_KERNELS)

// band and level (as a double) of every emission parameter, in LDS; all threads of the workgroup call
__device__ __forceinline__ void hml_rg_tables(const hml_model* __restrict__ mdl, const hml_band_edges& edges, uint8_t* band_of, double* level_of) {
    const int P = mdl->P < HML_CAP_K ? mdl->P : HML_CAP_K;
    for (int p = threadIdx.x; p < P; p += blockDim.x) {
        const float mu = mdl->mu[p];
        band_of[p] = (uint8_t)hml_band_of(edges, mu);
        level_of[p] = (double)mu;
    }
    __syncthreads();
}

// K14 regions_chunks - workgroup = chunk, thread = block.  A chunk's totals are added over a tree that the chunk alone fixes:
// a butterfly over the 64 lanes of a wavefront (both partners add the same two numbers, so every lane holds the same sum),
// then the four wavefronts' sums in order.
HML_KERNEL __launch_bounds__(256) void hml_k_regions_chunks(const int16_t* __restrict__ q, const uint32_t* __restrict__ starts,
                                                            const hml_model* __restrict__ mdl, const hml_band_edges edges,
                                                            hml_regions_chunks ch) {
    if (mdl->halted != 0u) return;   // (hml_state.h: the sweep did not happen; it is counted when it runs again)
    __shared__ uint8_t band_of[HML_CAP_K];
    __shared__ double level_of[HML_CAP_K];
    __shared__ uint32_t s_start[HML_RG_CHUNK + 1];
    __shared__ int16_t s_q[HML_RG_CHUNK + 1];
    __shared__ uint32_t w_cnt[4][1 + HML_MAX_D];
    __shared__ double w_lev[4][HML_MAX_D];
    hml_rg_tables(mdl, edges, band_of, level_of);
    const uint32_t B = mdl->B;
    const uint32_t T = mdl->T;
    const int D = mdl->D < HML_MAX_D ? mdl->D : HML_MAX_D;
    const uint32_t n_chunks = (B + HML_RG_CHUNK - 1u) >> HML_RG_SHIFT;
    const uint32_t tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    for (uint32_t c = blockIdx.x; c < n_chunks && c < ch.stride; c += gridDim.x) {
        const uint32_t b = (c << HML_RG_SHIFT) + tid;
        // s_q[i] = the state of block (first of the chunk) - 1 + i, s_start[i] = the start of block (first of the chunk) + i
        if (b < B) { s_q[tid + 1] = q[b]; s_start[tid] = starts[b]; }
        if (tid == 0) {
            s_q[0] = b > 0u ? q[b - 1u] : (int16_t)-1;
            const uint32_t after = b + HML_RG_CHUNK;
            s_start[HML_RG_CHUNK] = after < B ? starts[after] : T;
        }
        __syncthreads();
        uint32_t cnt[1 + HML_MAX_D];
        double lev[HML_MAX_D];
#pragma unroll
        for (int k = 0; k < 1 + HML_MAX_D; ++k) cnt[k] = 0u;
#pragma unroll
        for (int d = 0; d < HML_MAX_D; ++d) lev[d] = 0.0;
        if (b < B) {
            const int st = s_q[tid + 1], prev = s_q[tid];
            const uint32_t next = (b + 1u < B) ? s_start[tid + 1] : T;
            const double len = (double)(next - s_start[tid]);
            cnt[0] = (prev >= 0 && st != prev) ? 1u : 0u;
#pragma unroll
            for (int d = 0; d < HML_MAX_D; ++d) {
                if (d < D) {
                    const int p = mdl->map[st][d];
                    lev[d] = len * level_of[p];
                    cnt[1 + d] = (prev >= 0 && band_of[p] != band_of[mdl->map[prev][d]]) ? 1u : 0u;
                }
            }
        }
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
#pragma unroll
            for (int k = 0; k < 1 + HML_MAX_D; ++k) if (k < 1 + D) cnt[k] += __shfl_xor(cnt[k], m);
#pragma unroll
            for (int d = 0; d < HML_MAX_D; ++d) if (d < D) lev[d] += __shfl_xor(lev[d], m);   // (D is the same in every lane)
        }
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < 1 + HML_MAX_D; ++k) w_cnt[wave][k] = cnt[k];
#pragma unroll
            for (int d = 0; d < HML_MAX_D; ++d) w_lev[wave][d] = lev[d];
        }
        __syncthreads();
        if ((int)tid < 1 + D) ch.cnt[(uint64_t)tid * ch.stride + c] = ((w_cnt[0][tid] + w_cnt[1][tid]) + w_cnt[2][tid]) + w_cnt[3][tid];
        if ((int)tid < D) ch.lev[(uint64_t)tid * ch.stride + c] = ((w_lev[0][tid] + w_lev[1][tid]) + w_lev[2][tid]) + w_lev[3][tid];
        __syncthreads();
    }
}

// exclusive sums of one row's n totals, in place: the tree of hml_k_scan_chunks (hml_k_scan.h) - 1024 pieces of
// ceil(n / 1024) entries, each added up from zero, ten doubling steps over the pieces, and a piece runs on from the sum of
// the pieces before it - with n taken from the model instead of the launch
template <typename Acc>
__device__ __forceinline__ void hml_rg_scan_row(Acc* __restrict__ cs, uint32_t n, Acc* part) {
    const uint32_t tid = threadIdx.x;
    const uint32_t per = (n + 1023u) / 1024u;
    const uint32_t a = (uint64_t)tid * per < n ? tid * per : n;
    const uint32_t b = (a + per < n) ? a + per : n;
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

// K15 regions_scan - grid (1 + 2 D), or (1 + D) without edges: a row a workgroup
HML_KERNEL __launch_bounds__(1024) void hml_k_regions_scan(const hml_model* __restrict__ mdl, hml_regions_chunks ch) {
    if (mdl->halted != 0u) return;
    __shared__ double part[1024];
    const int D = mdl->D < HML_MAX_D ? mdl->D : HML_MAX_D;
    uint32_t n = (mdl->B + HML_RG_CHUNK - 1u) >> HML_RG_SHIFT;
    if (n > ch.stride) n = ch.stride;
    // rows: the D level sums, the state changes, the D band changes (launched only with edges: nobody reads them otherwise)
    const int row = blockIdx.x;
    if (row < D) hml_rg_scan_row<double>(ch.lev + (uint64_t)row * ch.stride, n, part);
    else if (row < 1 + 2 * D) hml_rg_scan_row<uint32_t>(ch.cnt + (uint64_t)(row - D) * ch.stride, n, reinterpret_cast<uint32_t*>(part));
}

// the last block b of [0, B) with starts[b] <= p, by the whole wavefront: every round the 64 lanes probe 64 evenly spaced
// blocks of the range that is left, and a ballot tells how many of them start at or before p (B = 2^30: 5 dependent rounds
// of loads where a binary search takes 30).  starts[0] = 0 <= p throughout.
__device__ __forceinline__ uint32_t hml_rg_block_of(const uint32_t* __restrict__ starts, uint32_t B, uint32_t p, int lane) {
    uint32_t lo = 0u, hi = B;   // the answer is in [lo, hi)
    while (hi - lo > 1u) {
        const uint32_t step = (hi - lo + 63u) >> 6;
        const uint64_t at = (uint64_t)lo + (uint64_t)lane * step;
        const bool le = at < hi && starts[at] <= p;
        const int n_le = __popcll(__ballot(le));   // (lane 0 probes `lo`: at least one)
        const uint32_t first = lo + (uint32_t)(n_le > 0 ? n_le - 1 : 0) * step;
        hi = (hi - first > step) ? first + step : hi;
        lo = first;
    }
    return lo;
}

// K16 regions_accumulate - a wavefront per region.  Region r belongs to one wavefront of a launch and the launches of a
// chain are ordered by its stream, so its accumulators take plain read-modify-writes (the argument of hml_b_record).
HML_KERNEL __launch_bounds__(256) void hml_k_regions_accumulate(const int16_t* __restrict__ q, const uint32_t* __restrict__ starts,
                                                                hml_model* __restrict__ mdl, const hml_band_edges edges,
                                                                const hml_regions_chunks ch, const uint32_t* __restrict__ rg_start,
                                                                const uint32_t* __restrict__ rg_end, uint32_t n_regions,
                                                                hml_regions_acc acc) {
    if (mdl->halted != 0u) return;
    __shared__ uint8_t band_of[HML_CAP_K];
    __shared__ double level_of[HML_CAP_K];
    hml_rg_tables(mdl, edges, band_of, level_of);
    const uint32_t B = mdl->B;
    const uint32_t T = mdl->T;
    const int D = mdl->D < HML_MAX_D ? mdl->D : HML_MAX_D;
    const int nbands = edges.n + 1;
    const int ncol = edges.n > 0 ? D * nbands : 0;
    const int lane = threadIdx.x & 63;
    const uint32_t waves = (gridDim.x * blockDim.x) >> 6;
    if (B != 0u) {
        for (uint32_t r = (blockIdx.x * blockDim.x + threadIdx.x) >> 6; r < n_regions; r += waves) {
            const uint32_t a = rg_start[r], e = rg_end[r];
            if (!(a < e && e <= T)) continue;   // (never: hml_set_regions and the first recorded sweep refuse such a region)
            const uint32_t ba = hml_rg_block_of(starts, B, a, lane);
            const uint32_t be = hml_rg_block_of(starts, B, e - 1u, lane);
            const uint32_t cba = ba >> HML_RG_SHIFT, cbe = be >> HML_RG_SHIFT;
            // the blocks of the region: those left of its first chunk [ba, a_last], the whole chunks cba + 1 ... cbe - 1, and,
            // when it reaches into another chunk, those of its last chunk [b_first, be]
            const uint32_t chunk_last = (cba << HML_RG_SHIFT) + (HML_RG_CHUNK - 1u);
            const uint32_t a_last = be < chunk_last ? be : chunk_last;
            const bool spans = cbe > cba;
            const uint32_t b_first = cbe << HML_RG_SHIFT;
            uint32_t cnt[2][1 + HML_MAX_D];
            double lev[2][HML_MAX_D];
#pragma unroll
            for (int part = 0; part < 2; ++part) {
#pragma unroll
                for (int k = 0; k < 1 + HML_MAX_D; ++k) cnt[part][k] = 0u;
#pragma unroll
                for (int d = 0; d < HML_MAX_D; ++d) lev[part][d] = 0.0;
                // (at most one chunk of blocks: four per lane, then the butterfly - an order that (ba, be) fixes)
                const uint32_t from = part == 0 ? ba : b_first;
                const uint32_t to = part == 0 ? a_last : be;
                if (part == 0 || spans) {
                    for (uint64_t b64 = (uint64_t)from + lane; b64 <= to; b64 += 64u) {
                        const uint32_t b = (uint32_t)b64;
                        const int st = q[b];
                        const uint32_t s0 = starts[b];
                        const uint32_t s1 = (b + 1u < B) ? starts[b + 1u] : T;
                        const double ovl = (double)((s1 < e ? s1 : e) - (s0 > a ? s0 : a));
                        const int prev = b > ba ? (int)q[b - 1u] : -1;   // (a change AT ba lies outside (ba, be])
                        cnt[part][0] += (prev >= 0 && st != prev) ? 1u : 0u;
#pragma unroll
                        for (int d = 0; d < HML_MAX_D; ++d) {
                            if (d < D) {
                                const int p = mdl->map[st][d];
                                lev[part][d] += ovl * level_of[p];
                                cnt[part][1 + d] += (prev >= 0 && band_of[p] != band_of[mdl->map[prev][d]]) ? 1u : 0u;
                            }
                        }
                    }
                }
#pragma unroll
                for (int m = 1; m < 64; m <<= 1) {
#pragma unroll
                    for (int k = 0; k < 1 + HML_MAX_D; ++k) cnt[part][k] += __shfl_xor(cnt[part][k], m);
#pragma unroll
                    for (int d = 0; d < HML_MAX_D; ++d) if (d < D) lev[part][d] += __shfl_xor(lev[part][d], m);
                }
            }
            if (lane == 0) {
                const uint64_t hi_at = cbe, lo_at = (uint64_t)cba + 1u;   // (exclusive sums: [hi] - [lo] = chunks lo ... hi - 1)
                const uint32_t nb = cnt[0][0] + (spans ? ch.cnt[hi_at] - ch.cnt[lo_at] : 0u) + cnt[1][0];
                acc.whole[r] += nb == 0u ? 1ull : 0ull;
                acc.breaks_sum[r] += (unsigned long long)nb;
                acc.breaks_sq[r] = hml_sat_add_u64(acc.breaks_sq[r], (unsigned long long)nb * (unsigned long long)nb);
                const double len = (double)(e - a);
                const int16_t st_a = q[ba];
#pragma unroll
                for (int d = 0; d < HML_MAX_D; ++d) {
                    if (d < D) {
                        const uint64_t row = (uint64_t)d * ch.stride;
                        const double mid = spans ? ch.lev[row + hi_at] - ch.lev[row + lo_at] : 0.0;
                        const double m = ((lev[0][d] + mid) + lev[1][d]) / len;
                        acc.level_sum[(uint64_t)d * n_regions + r] += m;
                        acc.level_sq[(uint64_t)d * n_regions + r] += m * m;
                        if (ncol > 0) {
                            const uint64_t crow = (uint64_t)(1 + d) * ch.stride;
                            const uint32_t changes = cnt[0][1 + d] + (spans ? ch.cnt[crow + hi_at] - ch.cnt[crow + lo_at] : 0u) + cnt[1][1 + d];
                            if (changes == 0u) acc.inband[(uint64_t)r * ncol + d * nbands + band_of[mdl->map[st_a][d]]] += 1ull;
                        }
                    }
                }
            }
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&mdl->n_regions_recorded, 1ull);
}

#endif   // HML_REGIONS_KERNELS

#endif

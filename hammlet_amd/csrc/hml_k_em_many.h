// E-steps of many members at once (hml_em_fit_many, include/hml.h; hml_em_many_ref.h; DESIGN.md 3c, "EM from many starts").
//
// A member is a set of parameters over the context's blocks; its E-step is hml_expected_counts' under those parameters, word
// for word.  Nothing of the arithmetic is restated here: every kernel below is its single-member sibling of hml_k_posterior.h
// or hml_k_em.h with THE MEMBER AS GRID DIMENSION y - it picks the member's record, which holds the arguments the sibling
// takes, and calls the device function the sibling calls.  Grid dimension x is the sibling's.  The records of a group lie in
// one device array; everything a member reads or writes beyond the chain's own arrays (integral array, block starts) is its own,
// so members share nothing and no word of one depends on another or on how the batch is cut into groups.
//   model, tables   a workgroup per member: the member's floats into a scratch model beside the context's configuration, then
//             (a second launch) the tables of hml_k_post_tables from it (hml_vit_par_fill, A and pi widened)
//   first / verify / rerun / finish   the smoothing's four (the scheme of hml_k_chunks.h), per direction; the counts lie per member in
//             one array the host reads in one copy per round; a round's repair launch covers the stale runs of all members
//             (a member with none has no lanes), the finishing launch has a wavefront per member (one without stale chunks
//             returns)
//   degenerate, ltree    the count of bad(c_b) - hml_k_post_combine's, without gamma and the call - and the tree over l_b
//   norm, reduce_small<8|16>, reduce, tree   the E-step's
//   gather    a member's results - the columns' roots, gamma_0, loglik and the three counts - into one row for one copy
#ifndef HML_K_EM_MANY_H
#define HML_K_EM_MANY_H

#include "hml_k_em.h"

// the words a member's kernels count in
enum { HML_EMM_W_WALKED = 0, HML_EMM_W_DEGENERATE = 1, HML_EMM_W_XI_BAD = 2, HML_EMM_WORDS = 3 };

struct hml_em_many_rec {
    hml_post_args dir[2];        // forward, backward (entry, exit, match and heads are used by one after the other)
    hml_em_args em;
    const float* floats;         // the member's mean_var[2 P], A[K K], pi[K]
    hml_model* mdl;              // scratch: what hml_vit_par_fill reads
    hml_vit_par* par;
    double *A, *pi;              // the widened tables (dir[].A, dir[].pi read them)
    uint8_t* match;              // [n_chunks]
    uint32_t* heads;             // [n_chunks]
    uint32_t* cnt;               // [2]: stale chunks, heads of their runs
    unsigned long long* words;   // [HML_EMM_WORDS]
    double* lt[2];               // the tree over l_b: levels 1, 2 (the levels above alternate between them)
    double* pt[2];               // the columns' trees: level 1 (= em.part), level 2
    double* X;                   // [B], K > 16 only
    double* result;              // [ncols + K + 4]: columns, first, loglik, walked, degenerate, xi_degenerate (the last three as words)
};

// the fields of the model hml_vit_par_fill reads: the context's configuration, the member's parameters
HML_KERNEL __launch_bounds__(256) void hml_k_em_many_model(const hml_model* __restrict__ ctx_mdl, const hml_em_many_rec* __restrict__ recs) {
    const hml_em_many_rec& r = recs[blockIdx.y];
    const int tid = threadIdx.x, K = ctx_mdl->K, P = ctx_mdl->P;
    hml_model* const m = r.mdl;
    if (tid == 0) {
        m->K = K; m->D = ctx_mdl->D; m->P = P; m->self_trans = ctx_mdl->self_trans; m->T = ctx_mdl->T; m->B = ctx_mdl->B;
    }
    if (tid < P) { m->mu[tid] = r.floats[2 * tid]; m->var[tid] = r.floats[2 * tid + 1]; }
    if (tid < K) {
        m->pi[tid] = r.floats[2 * P + K * K + tid];
        for (int d = 0; d < HML_MAX_D; ++d) m->map[tid][d] = ctx_mdl->map[tid][d];
    }
    for (int i = tid; i < K * K; i += 256) m->A[i] = r.floats[2 * P + i];
}
// hml_k_post_tables per member, from the model the kernel above has left (a launch of its own: the fill reads through
// read-only pointers)
HML_KERNEL __launch_bounds__(256) void hml_k_em_many_tables(const hml_em_many_rec* __restrict__ recs) {
    const hml_em_many_rec& r = recs[blockIdx.y];
    const hml_model* const m = r.mdl;
    const int tid = threadIdx.x, K = m->K;
    hml_vit_par_fill(m, r.par, tid);
    if (tid < K) r.pi[tid] = (double)m->pi[tid];
    for (int i = tid; i < K * K; i += 256) r.A[i] = (double)m->A[i];
}

template <int KM, int DIR>
HML_KERNEL __launch_bounds__(64) void hml_k_em_many_first(const hml_em_many_rec* __restrict__ recs) {
    extern __shared__ double hml_post_lds[];
    const hml_post_args a = recs[blockIdx.y].dir[DIR];
    hml_post_stage(a, a.par->K, hml_post_lds);
    const uint32_t x = blockIdx.x * 64u + threadIdx.x;
    if (x >= a.n_chunks) return;
    hml_post_run_chunk<KM, DIR>(a, hml_post_lds, x, nullptr);
}

// hml_chunk_verify per member
HML_KERNEL __launch_bounds__(256) void hml_k_em_many_verify(const hml_em_many_rec* __restrict__ recs, int dir, int K) {
    const hml_em_many_rec& r = recs[blockIdx.y];
    hml_chunk_verify(r.dir[dir].entry, r.dir[dir].exitv, K, r.dir[dir].n_chunks, r.match, r.heads, r.cnt, r.cnt + 1);
}

// grid x covers the greatest number of heads of the round
template <int KM, int DIR>
HML_KERNEL __launch_bounds__(64) void hml_k_em_many_rerun(const hml_em_many_rec* __restrict__ recs) {
    extern __shared__ double hml_post_lds[];
    const hml_em_many_rec& r = recs[blockIdx.y];
    const hml_post_args a = r.dir[DIR];
    const uint32_t n_heads = r.cnt[1];
    if (blockIdx.x * 64u >= n_heads) return;   // (the whole workgroup)
    hml_post_stage(a, a.par->K, hml_post_lds);
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n_heads) return;
    auto run = [&](uint32_t x, const double* from) { hml_post_run_chunk<KM, DIR>(a, hml_post_lds, x, from); };
    hml_chunk_rerun_walk(run, a.entry, a.exitv, a.par->K, a.n_chunks, r.heads[i], r.match);
}

template <int KM, int DIR>
HML_KERNEL __launch_bounds__(64) void hml_k_em_many_finish(const hml_em_many_rec* __restrict__ recs) {
    extern __shared__ double hml_post_lds[];
    const hml_em_many_rec& r = recs[blockIdx.y];
    if (r.cnt[0] == 0u || blockIdx.x != 0u || blockDim.x != 64u) return;   // (the whole workgroup)
    const hml_post_args a = r.dir[DIR];
    hml_post_stage(a, a.par->K, hml_post_lds);
    auto run = [&](uint32_t x, const double* from) { hml_post_run_chunk<KM, DIR>(a, hml_post_lds, x, from); };
    hml_chunk_finish_walk(run, a.entry, a.exitv, a.par->K, a.n_chunks, r.match, r.words + HML_EMM_W_WALKED);
}

HML_KERNEL __launch_bounds__(256) void hml_k_em_many_degenerate(const hml_em_many_rec* __restrict__ recs, uint32_t B) {
    const hml_em_many_rec& r = recs[blockIdx.y];
    const double* const cval = r.dir[0].cval;
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t b = blockIdx.x * blockDim.x + threadIdx.x; b < B; b += stride)
        if (hml_post_bad(cval[b])) atomicAdd(r.words + HML_EMM_W_DEGENERATE, 1ull);
}

// level k + 1 of the tree over l_b from level k (level 0: l_b itself), n values at level k
HML_KERNEL __launch_bounds__(256) void hml_k_em_many_ltree(const hml_em_many_rec* __restrict__ recs, int k, uint64_t n) {
    const hml_em_many_rec& r = recs[blockIdx.y];
    hml_post_tree_level(k == 0 ? r.dir[0].ell : r.lt[(k - 1) & 1], n, r.lt[k & 1]);
}

template <int KM>
HML_KERNEL __launch_bounds__(64) void hml_k_em_many_norm(const hml_em_many_rec* __restrict__ recs) {
    extern __shared__ double hml_post_lds[];
    const hml_em_many_rec& r = recs[blockIdx.y];
    const hml_post_args a = r.dir[0];
    hml_post_stage(a, a.par->K, hml_post_lds);
    hml_em_norm_block<KM>(a, hml_post_lds, r.em.alpha, r.em.beta, r.X, r.words + HML_EMM_W_XI_BAD);
}

HML_KERNEL __launch_bounds__(256) void hml_k_em_many_reduce(const hml_em_many_rec* __restrict__ recs) {
    const hml_em_args a = recs[blockIdx.y].em;
    hml_em_reduce_group(a);
}
template <int KS>
HML_KERNEL __launch_bounds__(64) void hml_k_em_many_reduce_small(const hml_em_many_rec* __restrict__ recs) {
    const hml_em_many_rec& r = recs[blockIdx.y];
    const hml_em_args a = r.em;
    hml_em_reduce_small_group<KS>(a, r.words + HML_EMM_W_XI_BAD);
}

// level k + 2 of the columns' trees from level k + 1 (k = 0: from the level `reduce` wrote)
HML_KERNEL __launch_bounds__(256) void hml_k_em_many_tree(const hml_em_many_rec* __restrict__ recs, int k, uint64_t n_x, uint64_t n_o, uint32_t ncols, uint32_t KK) {
    const hml_em_many_rec& r = recs[blockIdx.y];
    hml_em_tree_level(r.pt[k & 1], n_x, n_o, ncols, KK, r.pt[(k + 1) & 1]);
}

// l_levels, p_levels: the levels the two trees took (where their roots lie)
HML_KERNEL __launch_bounds__(256) void hml_k_em_many_gather(const hml_em_many_rec* __restrict__ recs, int l_levels, int p_levels, uint32_t ncols, int K) {
    const hml_em_many_rec& r = recs[blockIdx.y];
    const double* const cols = r.pt[p_levels & 1];
    double* const out = r.result;
    for (uint32_t i = threadIdx.x; i < ncols; i += blockDim.x) out[i] = cols[i];
    for (int i = threadIdx.x; i < K; i += blockDim.x) out[ncols + i] = r.em.first[i];
    if (threadIdx.x == 0) {
        out[ncols + K] = l_levels == 0 ? r.dir[0].ell[0] : r.lt[(l_levels - 1) & 1][0];
        for (int w = 0; w < HML_EMM_WORDS; ++w) out[ncols + K + 1 + w] = hml_u2d(r.words[w]);
    }
}

#endif

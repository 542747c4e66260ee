// libhammlet_hip.so - exact inference under the chain's current parameters, over its current blocks (include/hml.h): the most
// probable path (hml_viterbi*), the state posteriors and log p(y | theta) (hml_posterior*), the E-step's expected counts and
// the fits built on them (hml_expected_counts, hml_em_*, hml_em_fit_many), and the exact breakpoint and region posteriors
// (hml_posterior_breaks / _regions / _pair_terms), independent draws of whole paths (hml_posterior_sample*), and the exact
// breakpoint-count and state-avoidance posteriors per region (hml_posterior_region_counts).  Nothing here reads what a recorder wrote - those read-outs are
// hml_readout.hip's - and nothing runs inside a sweep: the chain is only read, every call owns its device memory for its own
// length, and the context keeps the launch geometry and a few numbers about the last call (hml_ctx::vit, post, em_many).
#include <limits>
#include <type_traits>

#include "hml_readout_shared.hpp"   // (scan_rows, model_fault, merge_runs; it brings hml_capi_shared.hpp)
#include "hml_em_ref.h"
#include "hml_em_many_ref.h"
// (each launched from this object alone)
#include "hml_k_viterbi.h"
#include "hml_k_posterior.h"
#include "hml_k_em.h"
#include "hml_k_em_many.h"
#include "hml_k_pairs.h"   // (it brings hml_pairs_ref.h)
#include "hml_k_sample.h"   // (it brings hml_sample_ref.h)
#include "hml_k_counts.h"   // (it brings hml_counts_ref.h)

// ---------------------------------------------------------------------------------------- what the passes share
// f(std::integral_constant<int, KM>()) for the number of states the kernels keep a recursion's vector for
template <class F>
static void by_states(int K, F f) {
    if (K <= 8) f(std::integral_constant<int, 8>());
    else if (K <= 16) f(std::integral_constant<int, 16>());
    else f(std::integral_constant<int, HML_CAP_K>());
}

// a pass's geometry over B blocks: its options, 0 meaning the default
struct chunk_geom { uint32_t L, W, n_chunks; };
static chunk_geom chunk_geom_of(const hml_ctx::chunked_pass& p, uint32_t default_L, uint32_t default_W, uint32_t B) {
    chunk_geom g;
    g.L = p.L ? p.L : default_L;
    g.W = p.W ? p.W : default_W;
    g.n_chunks = (uint32_t)(((uint64_t)B + g.L - 1u) / g.L);
    return g;
}

// The tables of a pass on the device: the parameters, and the transition and initial terms - fixed-point scores of 8 bytes for
// the decode (hml_k_vit_tables), A and pi in double for the smoothing (hml_k_post_tables).
struct infer_tables { DevBuf par, trans, init; };

// a pass may begin: the model fetched, no device error in it, a settled chain with blocks (`who`: the entry point the messages name)
static int infer_ready(hml_ctx* c, const char* who, hml_model* m) {
    if (int r = fetch_model(c, m)) return r;
    if (int r = model_fault(*m)) return r;
    if (m->halted) return set_err(HML_ERR_ARG, std::string(who) + ": the chain is halted; settle it with hml_sync first");
    if (m->B == 0) return set_err(HML_ERR_ARG, std::string(who) + ": no blocks yet: run a sweep or hml_create_blocks first");
    return 0;
}
// how a pass begins: that, and its tables on the device by `tables_kernel`
template <typename T>
static int infer_begin(hml_ctx* c, const char* who, void (*tables_kernel)(const hml_model*, hml_vit_par*, T*, T*), infer_tables& t, uint32_t* B_out) {
    static_assert(sizeof(T) == 8, "the tables hold 8-byte terms");
    hml_model m; if (int r = infer_ready(c, who, &m)) return r;
    const int K = c->K;
    HIPCHK(t.par.alloc(sizeof(hml_vit_par)));
    HIPCHK(t.trans.alloc((uint64_t)K * K * sizeof(T)));
    HIPCHK(t.init.alloc((uint64_t)K * sizeof(T)));
    hipLaunchKernelGGL(tables_kernel, dim3(1), dim3(256), 0, c->stream, c->d_mdl.get(), t.par.as<hml_vit_par>(), t.trans.as<T>(), t.init.as<T>());
    KLAUNCH_CHECK();
    *B_out = m.B;
    return 0;
}

// What every chunked pass does behind its first run: verify; while chunks are stale and rounds are left, rerun them in
// parallel; the single lane finishes what the rounds leave.  verify(&stale, &heads) zeroes the counters, launches the verify
// kernel and brings the counters back - one copy and one wait per round - giving the number of stale chunks and the number of
// heads of their runs (of a batch: the sum over members, the greatest over members); rerun(heads) and finish() launch.
struct repair_outcome { uint64_t stale_first = 0, rounds = 0; bool finished = false; };
template <class Verify, class Rerun, class Finish>
static int repair_rounds(uint32_t rounds, Verify verify, Rerun rerun, Finish finish, repair_outcome& out) {
    uint64_t stale = 0;
    for (uint32_t round = 0;; ++round) {
        uint32_t heads = 0;
        if (int r = verify(&stale, &heads)) return r;
        if (round == 0) out.stale_first = stale;
        if (stale == 0 || round >= rounds) break;
        rerun(heads);
        KLAUNCH_CHECK();
        out.rounds = round + 1u;
    }
    out.finished = stale != 0;
    if (!out.finished) return 0;
    finish();
    KLAUNCH_CHECK();
    return 0;
}
// verify of one pass: entry against exit rows (long long or double, compared as words); the counters are the first two 32-bit words of `words`
template <typename T>
static int verify_chunks(hml_ctx* c, const T* entry, const T* exitv, int K, uint32_t n_chunks, uint8_t* match, uint32_t* list, unsigned long long* words, uint64_t* stale,
                         uint32_t* heads) {
    uint32_t h_cnt[2] = {0, 0};   // stale chunks, heads of their runs
    HIPCHK(hipMemsetAsync(words, 0, sizeof h_cnt, c->stream));
    hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_k_chunk_verify<T>), dim3(grid_for(n_chunks, 256, 1, 4096)), dim3(256), 0, c->stream, entry, exitv, K, n_chunks, match, list,
                       (uint32_t*)words, (uint32_t*)words + 1);
    KLAUNCH_CHECK();
    HIPCHK(hipMemcpyAsync(h_cnt, words, sizeof h_cnt, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    *stale = h_cnt[0]; *heads = h_cnt[1];
    return 0;
}

// the runs of equal state over the blocks (keys d_q[B], starts the chain's block starts), as the segmentation read-out forms them
template <class Scatter>
static int block_runs(hml_ctx* c, const int16_t* d_q, uint32_t B, Scatter scatter, uint64_t* n_runs, uint64_t* run_len, int32_t* run_state) {
    std::vector<int16_t> state;
    if (int r = merge_runs(c->stream, d_q, B, (uint32_t)c->T, scatter, n_runs, run_len, state)) return r;
    if (run_len && run_state) std::copy(state.begin(), state.end(), run_state);
    return 0;
}

// ---------------------------------------------------------------------------------------- Viterbi decode (hml_k_viterbi.h)
// The jointly most probable state path over the current blocks under the current parameters.  Everything a decode allocates
// is local to the call: it goes on every path out, and the context keeps only the numbers of hml_viterbi_info.
struct vit_path { DevBuf q; long long score = 0; uint32_t B = 0; };

static int vit_begin(hml_ctx* c, infer_tables& t, uint32_t* B_out) { return infer_begin<long long>(c, "hml_viterbi", hml_k_vit_tables, t, B_out); }

// the decode: path (device, int16 per block) and score
static int vit_decode(hml_ctx* c, vit_path& out) {
    infer_tables t;
    uint32_t B = 0;
    if (int r = vit_begin(c, t, &B)) return r;
    const int K = c->K;
    const chunk_geom g = chunk_geom_of(c->vit, HML_VIT_DEFAULT_L, HML_VIT_DEFAULT_W, B);
    const uint32_t L = g.L, W = g.W, n_chunks = g.n_chunks;
    const uint32_t S = std::max<uint32_t>(1u, (uint32_t)std::ceil(std::sqrt((double)n_chunks)));   // chunks per group of the back-track
    const uint32_t n_groups = (n_chunks + S - 1u) / S;
    DevBuf b_entry, b_exit, b_psi, b_match, b_list, b_words, b_maps, b_gmaps, b_gend, b_cend;
    HIPCHK(b_entry.alloc((uint64_t)n_chunks * K * sizeof(long long)));
    HIPCHK(b_exit.alloc((uint64_t)n_chunks * K * sizeof(long long)));
    HIPCHK(b_psi.alloc((uint64_t)B * K));
    HIPCHK(b_match.alloc(n_chunks));
    HIPCHK(b_list.alloc((uint64_t)n_chunks * sizeof(uint32_t)));
    HIPCHK(b_words.alloc(4 * sizeof(unsigned long long)));   // [0] stale chunks and heads of their runs (32 bits each), [1] chunks the single lane ran, [2] the score
    HIPCHK(b_maps.alloc((uint64_t)n_chunks * K));
    HIPCHK(b_gmaps.alloc((uint64_t)n_groups * K));
    HIPCHK(b_gend.alloc(n_groups));
    HIPCHK(b_cend.alloc(n_chunks));
    HIPCHK(out.q.alloc((uint64_t)B * sizeof(int16_t)));
    uint8_t* const match = b_match.as<uint8_t>();
    uint32_t* const list = b_list.as<uint32_t>();
    unsigned long long* const words = b_words.as<unsigned long long>();
    hml_vit_args a;
    a.par = t.par.as<hml_vit_par>(); a.trans = t.trans.as<long long>(); a.init = t.init.as<long long>();
    a.ia = c->d_ia; a.starts = c->d_starts.get();
    a.L = L; a.W = W; a.n_chunks = n_chunks;
    a.entry = b_entry.as<long long>(); a.exitv = b_exit.as<long long>(); a.psi = b_psi.as<uint8_t>();
    HIPCHK(hipMemsetAsync(words, 0, 4 * sizeof(unsigned long long), c->stream));   // (the finishing walk adds to words[1])

    by_states(K, [&](auto km) { hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_k_vit_forward<km()>), dim3((n_chunks + 63u) / 64u), dim3(64), 0, c->stream, a); });
    KLAUNCH_CHECK();
    repair_outcome rep;
    auto verify = [&](uint64_t* stale, uint32_t* heads) { return verify_chunks(c, a.entry, a.exitv, K, n_chunks, match, list, words, stale, heads); };
    auto rerun = [&](uint32_t n_heads) {
        by_states(K, [&](auto km) { hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_k_vit_rerun<km()>), dim3((n_heads + 63u) / 64u), dim3(64), 0, c->stream, a, list, n_heads, match); });
    };
    auto finish = [&] {
        by_states(K, [&](auto km) { hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_k_vit_finish<km()>), dim3(1), dim3(64), 0, c->stream, a, match, words + 1); });
    };
    if (int r = repair_rounds(c->vit.rounds, verify, rerun, finish, rep)) return r;
    // back-track
    const dim3 cgrid((n_chunks + 63u) / 64u), ggrid((n_groups + 63u) / 64u);
    hipLaunchKernelGGL(hml_k_vit_chunk_maps, cgrid, dim3(64), 0, c->stream, a.psi, K, B, L, n_chunks, b_maps.as<uint8_t>());
    hipLaunchKernelGGL(hml_k_vit_group_maps, ggrid, dim3(64), 0, c->stream, b_maps.as<uint8_t>(), K, n_chunks, S, n_groups, b_gmaps.as<uint8_t>());
    hipLaunchKernelGGL(hml_k_vit_group_ends, dim3(1), dim3(64), 0, c->stream, a.exitv, b_gmaps.as<uint8_t>(), K, n_chunks, n_groups, b_gend.as<uint8_t>());
    hipLaunchKernelGGL(hml_k_vit_chunk_ends, ggrid, dim3(64), 0, c->stream, b_maps.as<uint8_t>(), b_gend.as<uint8_t>(), K, n_chunks, S, n_groups, b_cend.as<uint8_t>());
    hipLaunchKernelGGL(hml_k_vit_walk, cgrid, dim3(64), 0, c->stream, a.psi, b_cend.as<uint8_t>(), K, B, L, n_chunks, out.q.as<int16_t>());
    hipLaunchKernelGGL(hml_k_vit_score, dim3(grid_for(B, 256, 1, 4096)), dim3(256), 0, c->stream, a.par, a.trans, a.init, a.ia, a.starts, out.q.as<int16_t>(), words + 2);
    KLAUNCH_CHECK();
    unsigned long long h_words[4];
    HIPCHK(hipMemcpyAsync(h_words, words, sizeof h_words, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));   // (the scratch goes with this frame)
    out.score = (long long)h_words[2];
    out.B = B;
    c->vit.done = true;
    c->vit.chunks = n_chunks; c->vit.used_L = L; c->vit.used_W = W; c->vit.stale[0] = rep.stale_first; c->vit.rounds_run = rep.rounds; c->vit.walked = h_words[1];
    return 0;
}

extern "C" {

int hml_viterbi(hml_ctx* c, uint64_t* n_runs, uint64_t* run_len, int32_t* run_state, int64_t* score_fixed, double* score) {
    NEED_MODEL();
    if (!n_runs) return set_err(HML_ERR_ARG, "null argument");
    vit_path p;
    if (int r = vit_decode(c, p)) return r;
    if (score_fixed) *score_fixed = (int64_t)p.score;
    if (score) *score = (double)p.score / 1048576.0;
    auto scatter = [&](uint32_t n_chunks, const int32_t* d_rc, uint64_t, uint32_t* d_rs, int16_t* d_rq) {
        hipLaunchKernelGGL(hml_k_seg_run_scatter, dim3(n_chunks), dim3(256), 0, c->stream, p.q.as<int16_t>(), c->d_starts.get(), p.B, d_rc, d_rs, d_rq);
        return 0;
    };
    return block_runs(c, p.q.as<int16_t>(), p.B, scatter, n_runs, run_len, run_state);
}

int hml_viterbi_states(hml_ctx* c, int16_t* q) {
    NEED_MODEL();
    if (!q) return set_err(HML_ERR_ARG, "null argument");
    vit_path p;
    if (int r = vit_decode(c, p)) return r;
    HIPCHK(hipMemcpyAsync(q, p.q.get(), (uint64_t)p.B * sizeof(int16_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

int hml_viterbi_scores(hml_ctx* c, int64_t* emit, int64_t* trans, int64_t* init) {
    NEED_MODEL();
    infer_tables t;
    uint32_t B = 0;
    if (int r = vit_begin(c, t, &B)) return r;
    const int K = c->K;
    DevBuf b_emit;
    if (emit) {
        HIPCHK(b_emit.alloc((uint64_t)B * K * sizeof(long long)));
        hipLaunchKernelGGL(hml_k_vit_emit_table, dim3(grid_for(B, 256, 1, 16384)), dim3(256), 0, c->stream, t.par.as<hml_vit_par>(), c->d_ia, c->d_starts.get(), b_emit.as<long long>());
        KLAUNCH_CHECK();
        HIPCHK(hipMemcpyAsync(emit, b_emit.get(), (uint64_t)B * K * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    }
    if (trans) HIPCHK(hipMemcpyAsync(trans, t.trans.get(), (uint64_t)K * K * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    if (init) HIPCHK(hipMemcpyAsync(init, t.init.get(), (uint64_t)K * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

int hml_viterbi_info(hml_ctx* c, uint64_t* chunks, uint64_t* L, uint64_t* W, uint64_t* stale_chunks, uint64_t* rounds, uint64_t* serial_chunks) {
    if (!c) return set_err(HML_ERR_ARG, "null context");
    if (!c->vit.done) return set_err(HML_ERR_ARG, "hml_viterbi_info: nothing was decoded yet");
    if (chunks) *chunks = c->vit.chunks;
    if (L) *L = c->vit.used_L;
    if (W) *W = c->vit.used_W;
    if (stale_chunks) *stale_chunks = c->vit.stale[0];
    if (rounds) *rounds = c->vit.rounds_run;
    if (serial_chunks) *serial_chunks = c->vit.walked;
    return 0;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------- smoothing (hml_k_posterior.h)
// State posteriors per block, log p(y | theta) and the call with a confidence per run: the sum-product sibling of the decode
// above, with the same relation to the chain (read only) and to device memory (all of it local to the call).
struct post_result {
    DevBuf gamma, q, conf, alpha, cval, beta;   // gamma only if asked for
    double loglik = 0.0;
    uint64_t degenerate = 0;
    uint32_t B = 0;
};

static int post_begin(hml_ctx* c, infer_tables& t, uint32_t* B_out) { return infer_begin<double>(c, "hml_posterior", hml_k_post_tables, t, B_out); }

// The kernels' arguments from the context and the tables (parameters, A and pi in double).  The chunk fields as given - the
// kernels behind a smoothing pass need none; rows, c_b and l_b are the caller's to set.
static hml_post_args post_args_of(const hml_ctx* c, const hml_vit_par* par, const double* A, const double* pi, uint32_t L, uint32_t W, uint32_t n_chunks, double* entry,
                                  double* exitv) {
    hml_post_args a;
    a.par = par; a.A = A; a.pi = pi;
    a.ia = c->d_ia; a.starts = c->d_starts.get();
    a.L = L; a.W = W; a.n_chunks = n_chunks;
    a.entry = entry; a.exitv = exitv;
    a.rows = nullptr; a.cval = nullptr; a.ell = nullptr;
    return a;
}
static hml_post_args post_args_of(const hml_ctx* c, const infer_tables& t, uint32_t L = 0, uint32_t W = 0, uint32_t n_chunks = 0, double* entry = nullptr, double* exitv = nullptr) {
    return post_args_of(c, t.par.as<hml_vit_par>(), t.trans.as<double>(), t.init.as<double>(), L, W, n_chunks, entry, exitv);
}

// one direction: first run, then the repair rounds
template <int DIR>
static int post_direction(hml_ctx* c, const hml_post_args& a, int K, uint8_t* match, uint32_t* list, unsigned long long* words, repair_outcome& rep) {
    const size_t lds = ((size_t)K * K + K) * sizeof(double);
    by_states(K, [&](auto km) { hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_k_post_first<km(), DIR>), dim3((a.n_chunks + 63u) / 64u), dim3(64), lds, c->stream, a); });
    KLAUNCH_CHECK();
    auto verify = [&](uint64_t* stale, uint32_t* heads) { return verify_chunks(c, a.entry, a.exitv, K, a.n_chunks, match, list, words, stale, heads); };
    auto rerun = [&](uint32_t n_heads) {
        by_states(K, [&](auto km) {
            hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_k_post_rerun<km(), DIR>), dim3((n_heads + 63u) / 64u), dim3(64), lds, c->stream, a, list, n_heads, match);
        });
    };
    auto finish = [&] {
        by_states(K, [&](auto km) { hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_k_post_finish<km(), DIR>), dim3(1), dim3(64), lds, c->stream, a, match, words + 1); });
    };
    return repair_rounds(c->post.rounds, verify, rerun, finish, rep);
}

// The forward half: the tables, the rows alpha_b and c_b into `out`, l_b and the chunk scratch into `s` (the backward run uses
// entry, exit, match and list again).  The path sampler needs no more than this.
struct post_forward_scratch {
    DevBuf entry, exitv, match, list, words, ell;   // words: [0] stale chunks and heads (32 bits each), [1] chunks the single lane ran, [2] degenerate blocks, [3] log-likelihood
    uint32_t L = 0, W = 0, n_chunks = 0;
    repair_outcome rep;
};
static int post_forward(hml_ctx* c, post_result& out, infer_tables& t, post_forward_scratch& s) {
    uint32_t B = 0;
    if (int r = post_begin(c, t, &B)) return r;
    const int K = c->K;
    const chunk_geom g = chunk_geom_of(c->post, HML_POST_DEFAULT_L, HML_POST_DEFAULT_W, B);
    s.L = g.L; s.W = g.W; s.n_chunks = g.n_chunks;
    HIPCHK(out.alpha.alloc((uint64_t)B * K * sizeof(double)));
    HIPCHK(out.cval.alloc((uint64_t)B * sizeof(double)));
    HIPCHK(s.ell.alloc((uint64_t)B * sizeof(double)));
    HIPCHK(s.entry.alloc((uint64_t)s.n_chunks * K * sizeof(double)));
    HIPCHK(s.exitv.alloc((uint64_t)s.n_chunks * K * sizeof(double)));
    HIPCHK(s.match.alloc(s.n_chunks));
    HIPCHK(s.list.alloc((uint64_t)s.n_chunks * sizeof(uint32_t)));
    HIPCHK(s.words.alloc(4 * sizeof(unsigned long long)));
    HIPCHK(hipMemsetAsync(s.words.get(), 0, 4 * sizeof(unsigned long long), c->stream));
    hml_post_args a = post_args_of(c, t, s.L, s.W, s.n_chunks, s.entry.as<double>(), s.exitv.as<double>());
    a.rows = out.alpha.as<double>(); a.cval = out.cval.as<double>(); a.ell = s.ell.as<double>();
    out.B = B;
    return post_direction<0>(c, a, K, s.match.as<uint8_t>(), s.list.as<uint32_t>(), s.words.as<unsigned long long>(), s.rep);
}

// the whole computation; the rows alpha, c and beta stay in `out` for the probe, the tables in `t` for the E-step
static int post_compute(hml_ctx* c, bool want_gamma, post_result& out, infer_tables& t) {
    post_forward_scratch s;
    if (int r = post_forward(c, out, t, s)) return r;
    const int K = c->K;
    const uint32_t B = out.B, L = s.L, W = s.W, n_chunks = s.n_chunks;
    const uint64_t n1 = ((uint64_t)B + 63u) / 64u, n2 = (n1 + 63u) / 64u;   // the first two levels of the tree
    DevBuf b_t1, b_t2;
    DevBuf &b_entry = s.entry, &b_exit = s.exitv, &b_match = s.match, &b_list = s.list, &b_ell = s.ell;
    HIPCHK(out.beta.alloc((uint64_t)B * K * sizeof(double)));
    HIPCHK(b_t1.alloc(n1 * sizeof(double)));
    HIPCHK(b_t2.alloc(n2 * sizeof(double)));
    HIPCHK(out.q.alloc((uint64_t)B * sizeof(int16_t)));
    HIPCHK(out.conf.alloc((uint64_t)B * sizeof(double)));
    if (want_gamma) HIPCHK(out.gamma.alloc((uint64_t)B * K * sizeof(double)));
    unsigned long long* const words = s.words.as<unsigned long long>();

    hml_post_args a = post_args_of(c, t, L, W, n_chunks, b_entry.as<double>(), b_exit.as<double>());
    repair_outcome rep[2];
    rep[0] = s.rep;
    a.rows = out.beta.as<double>(); a.cval = nullptr; a.ell = nullptr;   // (entry, exit, match and list are used again)
    if (int r = post_direction<1>(c, a, K, b_match.as<uint8_t>(), b_list.as<uint32_t>(), words, rep[1])) return r;

    hipLaunchKernelGGL(hml_k_post_combine, dim3(grid_for(B, 256, 1, 16384)), dim3(256), 0, c->stream, out.alpha.as<double>(), out.beta.as<double>(), out.cval.as<double>(), K, B,
                       want_gamma ? out.gamma.as<double>() : nullptr, out.q.as<int16_t>(), out.conf.as<double>(), words + 2);
    // the tree over l_b: levels until one value is left
    const double* level = b_ell.as<double>();
    uint64_t n = B;
    double* bufs[2] = {b_t1.as<double>(), b_t2.as<double>()};
    for (int k = 0; n > 1; ++k) {
        double* const dst = bufs[k & 1];
        hipLaunchKernelGGL(hml_k_post_tree, dim3(grid_for((n + 63u) / 64u, 256, 1, 4096)), dim3(256), 0, c->stream, level, n, dst);
        level = dst;
        n = (n + 63u) / 64u;
    }
    KLAUNCH_CHECK();
    unsigned long long h_words[4];
    HIPCHK(hipMemcpyAsync(h_words, words, sizeof h_words, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(&out.loglik, level, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));   // (the scratch goes with this frame)
    out.degenerate = h_words[2];
    out.B = B;
    c->post.done = true;
    c->post.chunks = n_chunks; c->post.used_L = L; c->post.used_W = W; c->post.stale[0] = rep[0].stale_first; c->post.stale[1] = rep[1].stale_first;
    c->post.rounds_run = std::max(rep[0].rounds, rep[1].rounds); c->post.walked = (rep[0].finished || rep[1].finished) ? h_words[1] : 0;
    return 0;
}

static int post_compute(hml_ctx* c, bool want_gamma, post_result& out) {
    infer_tables t;
    return post_compute(c, want_gamma, out, t);
}

extern "C" {

int hml_posterior(hml_ctx* c, double* gamma, double* loglik, uint64_t* degenerate) {
    NEED_MODEL();
    post_result p;
    if (int r = post_compute(c, gamma != nullptr, p)) return r;
    if (gamma) {
        HIPCHK(hipMemcpyAsync(gamma, p.gamma.get(), (uint64_t)p.B * c->K * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    if (loglik) *loglik = p.loglik;
    if (degenerate) *degenerate = p.degenerate;
    return 0;
}

int hml_posterior_rle(hml_ctx* c, uint64_t* n_runs, uint64_t* run_len, int32_t* run_state, double* run_conf) {
    NEED_MODEL();
    if (!n_runs) return set_err(HML_ERR_ARG, "null argument");
    post_result p;
    if (int r = post_compute(c, false, p)) return r;
    // runs of equal state over the blocks, as hml_viterbi forms them, each with the minimum of its blocks' posteriors
    DevBuf b_rconf;   // (the minima are taken over the words of the doubles, from all bits set)
    auto scatter = [&](uint32_t n_chunks, const int32_t* d_rc, uint64_t R, uint32_t* d_rs, int16_t* d_rq) {
        HIPCHK(b_rconf.alloc(R * sizeof(double)));
        HIPCHK(hipMemsetAsync(b_rconf.get(), 0xff, R * sizeof(double), c->stream));
        hipLaunchKernelGGL(hml_k_post_run_scatter, dim3(n_chunks), dim3(256), 0, c->stream, p.q.as<int16_t>(), p.conf.as<double>(), c->d_starts.get(), p.B, d_rc, d_rs, d_rq,
                           b_rconf.as<unsigned long long>());
        if (run_conf) HIPCHK(hipMemcpyAsync(run_conf, b_rconf.get(), R * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        return 0;
    };
    return block_runs(c, p.q.as<int16_t>(), p.B, scatter, n_runs, run_len, run_state);
}

int hml_posterior_terms(hml_ctx* c, float* e, float* m, double* alpha, double* cval, double* beta) {
    NEED_MODEL();
    const int K = c->K;
    if (e || m) {
        infer_tables t;
        uint32_t B = 0;
        if (int r = post_begin(c, t, &B)) return r;
        DevBuf b_e, b_m;
        if (e) HIPCHK(b_e.alloc((uint64_t)B * K * sizeof(float)));
        if (m) HIPCHK(b_m.alloc((uint64_t)B * sizeof(float)));
        hipLaunchKernelGGL(hml_k_post_term_table, dim3(grid_for(B, 256, 1, 16384)), dim3(256), 0, c->stream, t.par.as<hml_vit_par>(), c->d_ia, c->d_starts.get(), b_e.as<float>(),
                           b_m.as<float>());
        KLAUNCH_CHECK();
        if (e) HIPCHK(hipMemcpyAsync(e, b_e.get(), (uint64_t)B * K * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        if (m) HIPCHK(hipMemcpyAsync(m, b_m.get(), (uint64_t)B * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    if (alpha || cval || beta || !(e || m)) {
        post_result p;
        if (int r = post_compute(c, false, p)) return r;
        if (alpha) HIPCHK(hipMemcpyAsync(alpha, p.alpha.get(), (uint64_t)p.B * K * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        if (cval) HIPCHK(hipMemcpyAsync(cval, p.cval.get(), (uint64_t)p.B * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        if (beta) HIPCHK(hipMemcpyAsync(beta, p.beta.get(), (uint64_t)p.B * K * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    return 0;
}

int hml_posterior_info(hml_ctx* c, uint64_t* chunks, uint64_t* L, uint64_t* W, uint64_t* stale_fwd, uint64_t* stale_bwd, uint64_t* rounds, uint64_t* serial_chunks) {
    if (!c) return set_err(HML_ERR_ARG, "null context");
    if (!c->post.done) return set_err(HML_ERR_ARG, "hml_posterior_info: nothing was computed yet");
    if (chunks) *chunks = c->post.chunks;
    if (L) *L = c->post.used_L;
    if (W) *W = c->post.used_W;
    if (stale_fwd) *stale_fwd = c->post.stale[0];
    if (stale_bwd) *stale_bwd = c->post.stale[1];
    if (rounds) *rounds = c->post.rounds_run;
    if (serial_chunks) *serial_chunks = c->post.walked;
    return 0;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------- expectation-maximisation (hml_k_em.h)
// The E-step's expected counts behind a smoothing pass, the M-step of hml_em_ref.h on the host, and the fit.  Device memory is
// local to a call, as the smoothing's is.

// a row of root columns (xi row-major, then occ[K], stay[K], sx[D][K], sxx[D][K]: hml_k_em.h) into the counts; one block has no pair
static void em_unpack_columns(const double* cols, int K, int D, uint32_t B, hml_em_counts& out) {
    const int KK = K * K;
    out.xi.assign(cols, cols + KK);
    if (B == 1u) out.xi.assign((size_t)KK, 0.0);
    out.occ.assign(cols + KK, cols + KK + K);
    out.stay.assign(cols + KK + K, cols + KK + 2 * K);
    out.sx.resize((size_t)K * D); out.sxx.resize((size_t)K * D);
    for (int j = 0; j < K; ++j)
        for (int d = 0; d < D; ++d) {
            out.sx[j * D + d] = cols[KK + (2 + d) * K + j];
            out.sxx[j * D + d] = cols[KK + (2 + D + d) * K + j];
        }
}

// the E-step: a smoothing pass, then the counts
static int em_estep(hml_ctx* c, hml_em_counts& out) {
    infer_tables t;
    post_result p;
    if (int r = post_compute(c, false, p, t)) return r;
    const int K = c->K, D = c->D, KK = K * K;
    const uint32_t B = p.B;
    const uint32_t ncols = (uint32_t)(KK + K * (2 + 2 * D));
    const uint64_t n1 = ((uint64_t)B + 63u) / 64u, n2 = (n1 + 63u) / 64u;
    DevBuf b_X, b_p1, b_p2, b_first, b_bad;
    const bool small = K <= 16;   // one wavefront per group, X_b computed where it is used (hml_k_em_reduce_small)
    if (!small) HIPCHK(b_X.alloc((uint64_t)B * sizeof(double)));
    HIPCHK(b_p1.alloc(n1 * ncols * sizeof(double)));
    HIPCHK(b_p2.alloc(n2 * ncols * sizeof(double)));
    HIPCHK(b_first.alloc((uint64_t)K * sizeof(double)));
    HIPCHK(b_bad.alloc(sizeof(unsigned long long)));
    HIPCHK(hipMemsetAsync(b_bad.get(), 0, sizeof(unsigned long long), c->stream));
    if (B > 1u && !small) {
        const hml_post_args a = post_args_of(c, t);
        by_states(K, [&](auto km) {
            hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_k_em_norm<km()>), dim3((B - 1u + 63u) / 64u), dim3(64), ((size_t)KK + K) * sizeof(double), c->stream, a, p.alpha.as<double>(),
                               p.beta.as<double>(), b_X.as<double>(), b_bad.as<unsigned long long>());
        });
        KLAUNCH_CHECK();
    }
    hml_em_args e;
    e.par = t.par.as<hml_vit_par>(); e.A = t.trans.as<double>(); e.ia = c->d_ia; e.starts = c->d_starts.get();
    e.alpha = p.alpha.as<double>(); e.beta = p.beta.as<double>(); e.X = b_X.as<double>();
    e.part = b_p1.as<double>(); e.first = b_first.as<double>();
    if (K <= 8) hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_k_em_reduce_small<8>), dim3((uint32_t)n1), dim3(64), 0, c->stream, e, b_bad.as<unsigned long long>());
    else if (small) hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_k_em_reduce_small<16>), dim3((uint32_t)n1), dim3(64), 0, c->stream, e, b_bad.as<unsigned long long>());
    else hipLaunchKernelGGL(hml_k_em_reduce, dim3((uint32_t)n1), dim3(256), 0, c->stream, e);
    // the upper levels of the trees: xi's has B - 1 leaves, the others' B
    const double* level = b_p1.as<double>();
    uint64_t n_x = ((uint64_t)B - 1u + 63u) / 64u, n_o = n1;
    double* bufs[2] = {b_p2.as<double>(), b_p1.as<double>()};
    for (int k = 0; n_o > 1; ++k) {
        double* const dst = bufs[k & 1];
        hipLaunchKernelGGL(hml_k_em_tree, dim3(grid_for(((n_o + 63u) / 64u) * ncols, 256, 1, 4096)), dim3(256), 0, c->stream, level, n_x, n_o, ncols, (uint32_t)KK, dst);
        level = dst;
        n_x = (n_x + 63u) / 64u; n_o = (n_o + 63u) / 64u;
    }
    KLAUNCH_CHECK();
    std::vector<double> cols(ncols);
    unsigned long long n_bad = 0;
    out.first.resize(K);
    HIPCHK(hipMemcpyAsync(cols.data(), level, (uint64_t)ncols * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(out.first.data(), b_first.get(), (uint64_t)K * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(&n_bad, b_bad.get(), sizeof n_bad, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));   // (the scratch goes with this frame)
    em_unpack_columns(cols.data(), K, D, B, out);
    out.loglik = p.loglik;
    out.degenerate = p.degenerate;
    out.xi_degenerate = n_bad;
    return 0;
}

// the context's float parameters and priors, as the M-step and the objective take them
struct em_params {
    std::vector<float> mv, A, pi;
    hml_em_prior pr;
    int P = 0, self_trans = 1;
};
static void em_params_of(const hml_model& m, int K, em_params& q);
static int em_fetch(hml_ctx* c, em_params& q) {
    hml_model m; if (int r = fetch_model(c, &m)) return r;
    em_params_of(m, c->K, q);
    return 0;
}
static void em_params_of(const hml_model& m, int K, em_params& q) {
    q.P = m.P; q.self_trans = m.self_trans != 0;
    q.mv.resize(2 * (size_t)m.P);
    for (int k = 0; k < m.P; ++k) { q.mv[2 * k] = m.mu[k]; q.mv[2 * k + 1] = m.var[k]; }
    q.A.assign(m.A, m.A + K * K);
    q.pi.assign(m.pi, m.pi + K);
    q.pr.alpha = (double)m.nig_prior[0]; q.pr.beta = (double)m.nig_prior[1]; q.pr.mu0 = (double)m.nig_prior[2]; q.pr.nu = (double)m.nig_prior[3];
    q.pr.a_off = (double)m.a_off; q.pr.a_diag = (double)m.a_diag; q.pr.pi_alpha = (double)m.pi_alpha;
}

// one E-step, the objective of the current parameters, and whether the E-step was degenerate
static int em_expect(hml_ctx* c, int use_prior, em_params& q, hml_em_counts& n, double* objective) {
    if (int r = em_estep(c, n)) return r;
    if (int r = em_fetch(c, q)) return r;
    *objective = hml_em_objective(c->K, q.P, use_prior, q.pr, n.loglik, q.mv.data(), q.A.data(), q.pi.data());
    return 0;
}
// the M-step and the installation of its result
static int em_maximise(hml_ctx* c, int use_prior, em_params& q, const hml_em_counts& n, uint64_t* kept) {
    *kept += hml_em_mstep(c->K, c->D, q.P, q.self_trans, use_prior, q.pr, n, q.mv.data(), q.A.data(), q.pi.data());
    return hml_set_parameters(c, q.mv.data(), q.A.data(), q.pi.data());
}

extern "C" {

int hml_expected_counts(hml_ctx* c, double* xi, double* first, double* stay, double* occ, double* sum, double* sum_sq, double* loglik, uint64_t* degenerate,
                        uint64_t* xi_degenerate) {
    NEED_MODEL();
    hml_em_counts n;
    if (int r = em_estep(c, n)) return r;
    if (xi) std::copy(n.xi.begin(), n.xi.end(), xi);
    if (first) std::copy(n.first.begin(), n.first.end(), first);
    if (stay) std::copy(n.stay.begin(), n.stay.end(), stay);
    if (occ) std::copy(n.occ.begin(), n.occ.end(), occ);
    if (sum) std::copy(n.sx.begin(), n.sx.end(), sum);
    if (sum_sq) std::copy(n.sxx.begin(), n.sxx.end(), sum_sq);
    if (loglik) *loglik = n.loglik;
    if (degenerate) *degenerate = n.degenerate;
    if (xi_degenerate) *xi_degenerate = n.xi_degenerate;
    return 0;
}

int hml_em_step(hml_ctx* c, int use_prior, double* objective_before, uint64_t* kept) {
    NEED_MODEL();
    em_params q;
    hml_em_counts n;
    double obj = 0.0;
    uint64_t k = 0;
    if (int r = em_expect(c, use_prior, q, n, &obj)) return r;
    if (int r = em_maximise(c, use_prior, q, n, &k)) return r;
    if (objective_before) *objective_before = obj;
    if (kept) *kept = k;
    return 0;
}

int hml_em_fit(hml_ctx* c, int use_prior, uint64_t max_steps, double rel_tol, double* trace, uint64_t* steps, int* reason, uint64_t* kept) {
    NEED_MODEL();
    uint64_t k_total = 0, k = 0;
    int why = HML_EM_MAX_STEPS;
    double last[2] = {0.0, 0.0};   // trace[k - 1], trace[k]
    for (;; ++k) {
        em_params q;
        hml_em_counts n;
        last[0] = last[1];
        if (int r = em_expect(c, use_prior, q, n, &last[1])) return r;
        if (trace) trace[k] = last[1];
        if (hml_em_stops(last[0], last[1], k, max_steps, rel_tol, n.degenerate + n.xi_degenerate, &why)) break;
        if (int r = em_maximise(c, use_prior, q, n, &k_total)) return r;
    }
    if (steps) *steps = k;
    if (reason) *reason = why;
    if (kept) *kept = k_total;
    return 0;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------- EM from many starts (hml_k_em_many.h)
// A batch of fits over the same blocks, each hml_set_parameters(start) + hml_em_fit word for word: the E-steps of the members
// still running go through one set of launches per group, the member being grid dimension y; objective, stopping rule and
// M-step are the header's functions per member on the host, as in hml_em_fit.  The context's parameters are not touched before
// the winner is installed.  Device memory is local to the call.
#define HML_EM_MANY_DEFAULT_BYTES (4ull << 30)   // of a group's device memory (hml_set_em_batch_bytes)

struct em_many_geom {
    int K = 0, D = 0, P = 0;
    uint32_t B = 0, L = 0, W = 0, n_chunks = 0, ncols = 0;
    uint64_t n1 = 0, n2 = 0, nfloats = 0, nresult = 0;
    bool small = false;
};
struct em_many_bufs {
    DevBuf alpha, beta, cval, ell, entry, exitv, match, heads, cnt, words, lt1, lt2, X, p1, p2, first, par, A, pi, mdl, floats, result, recs;
};
struct em_many_stats { uint64_t launch_sets = 0, stale[2] = {0, 0}, rounds = 0, walked = 0; };

// (array, bytes per member) in the order they are allocated
static std::vector<std::pair<DevBuf*, uint64_t>> em_many_layout(em_many_bufs& b, const em_many_geom& g) {
    const uint64_t B = g.B, K = g.K, dbl = sizeof(double);
    std::vector<std::pair<DevBuf*, uint64_t>> v = {
        {&b.alpha, B * K * dbl}, {&b.beta, B * K * dbl}, {&b.cval, B * dbl}, {&b.ell, B * dbl}, {&b.entry, (uint64_t)g.n_chunks * K * dbl},
        {&b.exitv, (uint64_t)g.n_chunks * K * dbl}, {&b.match, g.n_chunks}, {&b.heads, (uint64_t)g.n_chunks * sizeof(uint32_t)}, {&b.cnt, 2 * sizeof(uint32_t)},
        {&b.words, HML_EMM_WORDS * sizeof(unsigned long long)}, {&b.lt1, g.n1 * dbl}, {&b.lt2, g.n2 * dbl}, {&b.p1, g.n1 * g.ncols * dbl},
        {&b.p2, g.n2 * g.ncols * dbl}, {&b.first, K * dbl}, {&b.par, sizeof(hml_vit_par)}, {&b.A, K * K * dbl}, {&b.pi, K * dbl}, {&b.mdl, sizeof(hml_model)},
        {&b.floats, g.nfloats * sizeof(float)}, {&b.result, g.nresult * dbl}, {&b.recs, sizeof(hml_em_many_rec)}};
    if (!g.small) v.push_back({&b.X, B * dbl});
    return v;
}

// one direction of the smoothing for the first n records: the repair rounds with the member as grid dimension y, the counters
// of all members in one copy per round
template <int DIR>
static int em_many_direction(hml_ctx* c, const em_many_geom& g, em_many_bufs& b, uint32_t n, em_many_stats& st) {
    const hml_em_many_rec* const recs = b.recs.as<hml_em_many_rec>();
    const int K = g.K;
    const size_t lds = ((size_t)K * K + K) * sizeof(double);
    by_states(K, [&](auto km) { hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_k_em_many_first<km(), DIR>), dim3((g.n_chunks + 63u) / 64u, n), dim3(64), lds, c->stream, recs); });
    KLAUNCH_CHECK();
    std::vector<uint32_t> h_cnt(2 * (size_t)n);   // per member: stale chunks, heads of their runs
    auto verify = [&](uint64_t* stale, uint32_t* max_heads) {
        HIPCHK(hipMemsetAsync(b.cnt.get(), 0, h_cnt.size() * sizeof(uint32_t), c->stream));
        hipLaunchKernelGGL(hml_k_em_many_verify, dim3(grid_for(g.n_chunks, 256, 1, 4096), n), dim3(256), 0, c->stream, recs, DIR, K);
        KLAUNCH_CHECK();
        HIPCHK(hipMemcpyAsync(h_cnt.data(), b.cnt.get(), h_cnt.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        *stale = 0; *max_heads = 0;
        for (uint32_t i = 0; i < n; ++i) { *stale += h_cnt[2 * i]; *max_heads = std::max(*max_heads, h_cnt[2 * i + 1]); }
        return 0;
    };
    auto rerun = [&](uint32_t max_heads) {
        by_states(K, [&](auto km) { hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_k_em_many_rerun<km(), DIR>), dim3((max_heads + 63u) / 64u, n), dim3(64), lds, c->stream, recs); });
    };
    auto finish = [&] {
        by_states(K, [&](auto km) { hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_k_em_many_finish<km(), DIR>), dim3(1, n), dim3(64), lds, c->stream, recs); });
    };
    repair_outcome rep;
    if (int r = repair_rounds(c->post.rounds, verify, rerun, finish, rep)) return r;
    st.stale[DIR] += rep.stale_first;
    st.rounds = std::max(st.rounds, rep.rounds);
    return 0;
}

// The E-step of n members, whose floats (mean_var, A, pi per member) are h_floats: their result rows into h_result.
static int em_many_estep(hml_ctx* c, const em_many_geom& g, em_many_bufs& b, uint32_t n, const float* h_floats, double* h_result, em_many_stats& st) {
    const hml_em_many_rec* const recs = b.recs.as<hml_em_many_rec>();
    const int K = g.K;
    HIPCHK(hipMemcpyAsync(b.floats.get(), h_floats, (uint64_t)n * g.nfloats * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemsetAsync(b.words.get(), 0, (uint64_t)n * HML_EMM_WORDS * sizeof(unsigned long long), c->stream));
    hipLaunchKernelGGL(hml_k_em_many_model, dim3(1, n), dim3(256), 0, c->stream, c->d_mdl.get(), recs);
    hipLaunchKernelGGL(hml_k_em_many_tables, dim3(1, n), dim3(256), 0, c->stream, recs);
    KLAUNCH_CHECK();
    ++st.launch_sets;
    if (int r = em_many_direction<0>(c, g, b, n, st)) return r;
    if (int r = em_many_direction<1>(c, g, b, n, st)) return r;
    hipLaunchKernelGGL(hml_k_em_many_degenerate, dim3(grid_for(g.B, 256, 1, 16384), n), dim3(256), 0, c->stream, recs, g.B);
    int l_levels = 0, p_levels = 0;
    for (uint64_t m = g.B; m > 1; m = (m + 63u) / 64u, ++l_levels)
        hipLaunchKernelGGL(hml_k_em_many_ltree, dim3(grid_for((m + 63u) / 64u, 256, 1, 4096), n), dim3(256), 0, c->stream, recs, l_levels, m);
    KLAUNCH_CHECK();
    if (g.B > 1u && !g.small) {
        by_states(K, [&](auto km) {
            hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_k_em_many_norm<km()>), dim3((g.B - 1u + 63u) / 64u, n), dim3(64), ((size_t)K * K + K) * sizeof(double), c->stream, recs);
        });
        KLAUNCH_CHECK();
    }
    if (K <= 8) hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_k_em_many_reduce_small<8>), dim3((uint32_t)g.n1, n), dim3(64), 0, c->stream, recs);
    else if (g.small) hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_k_em_many_reduce_small<16>), dim3((uint32_t)g.n1, n), dim3(64), 0, c->stream, recs);
    else hipLaunchKernelGGL(hml_k_em_many_reduce, dim3((uint32_t)g.n1, n), dim3(256), 0, c->stream, recs);
    uint64_t n_x = ((uint64_t)g.B - 1u + 63u) / 64u, n_o = g.n1;
    for (; n_o > 1; ++p_levels) {
        hipLaunchKernelGGL(hml_k_em_many_tree, dim3(grid_for(((n_o + 63u) / 64u) * g.ncols, 256, 1, 4096), n), dim3(256), 0, c->stream, recs, p_levels, n_x, n_o, g.ncols,
                           (uint32_t)(K * K));
        n_x = (n_x + 63u) / 64u; n_o = (n_o + 63u) / 64u;
    }
    hipLaunchKernelGGL(hml_k_em_many_gather, dim3(1, n), dim3(256), 0, c->stream, recs, l_levels, p_levels, g.ncols, K);
    KLAUNCH_CHECK();
    HIPCHK(hipMemcpyAsync(h_result, b.result.get(), (uint64_t)n * g.nresult * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

// a member's result row as the counts em_estep returns
static void em_many_counts(const em_many_geom& g, const double* row, hml_em_counts& out, uint64_t* walked) {
    em_unpack_columns(row, g.K, g.D, g.B, out);
    const double* const tail = row + g.ncols;
    out.first.assign(tail, tail + g.K);
    out.loglik = tail[g.K];
    uint64_t w[HML_EMM_WORDS];
    memcpy(w, tail + g.K + 1, sizeof w);
    *walked = w[HML_EMM_W_WALKED];
    out.degenerate = w[HML_EMM_W_DEGENERATE];
    out.xi_degenerate = w[HML_EMM_W_XI_BAD];
}

// hml_set_parameters' refusal of a start, or "" if it takes it
static std::string em_many_refusal(int P, const float* mean_var) {
    for (int k = 0; k < P; ++k) {
        const float mean = mean_var[2 * k], var = mean_var[2 * k + 1];
        if (!std::isfinite(mean)) return "Mean (" + std::to_string(mean) + ") must be set to a finite value!";
        if (!std::isfinite(var)) return "Variance(" + std::to_string(var) + ") must be set to a finite value!";
        if (var <= 0) return "Variance (" + std::to_string(var) + ") must be positive!";
    }
    return "";
}

extern "C" {

int hml_em_fit_many(hml_ctx* c, uint64_t R, const float* mean_var, const float* A, const float* pi, int use_prior, uint64_t max_steps, double rel_tol, int install,
                    double* trace, uint64_t* steps, int* reason, uint64_t* kept, float* fit_mean_var, float* fit_A, float* fit_pi, double* objective, int64_t* best) {
    NEED_MODEL();
    if (R < 1u || R > HML_EM_MANY_MAX_R) return set_err(HML_ERR_ARG, "hml_em_fit_many: the number of members must be 1 ... " + std::to_string(HML_EM_MANY_MAX_R));
    if (!mean_var || !A || !pi) return set_err(HML_ERR_ARG, "null argument");
    hml_model m; if (int r = infer_ready(c, "hml_posterior", &m)) return r;
    em_many_geom g;
    g.K = c->K; g.D = c->D; g.P = m.P; g.B = m.B;
    const int K = g.K, KK = K * K, P = g.P;
    for (uint64_t r = 0; r < R; ++r) {
        const std::string why = em_many_refusal(P, mean_var + r * 2u * P);
        if (!why.empty()) return set_err(HML_ERR_MODEL, why + " (start " + std::to_string(r) + ")");
    }
    em_params q0;
    em_params_of(m, K, q0);
    const chunk_geom cg = chunk_geom_of(c->post, HML_POST_DEFAULT_L, HML_POST_DEFAULT_W, g.B);
    g.L = cg.L; g.W = cg.W; g.n_chunks = cg.n_chunks;
    g.ncols = (uint32_t)(KK + K * (2 + 2 * g.D));
    g.n1 = ((uint64_t)g.B + 63u) / 64u; g.n2 = (g.n1 + 63u) / 64u;
    g.nfloats = 2u * P + KK + K;
    g.nresult = (uint64_t)g.ncols + K + 1u + HML_EMM_WORDS;
    g.small = K <= 16;

    // the group: as many members as the byte budget holds
    em_many_bufs b;
    const auto layout = em_many_layout(b, g);
    uint64_t member_bytes = 0;
    for (const auto& e : layout) member_bytes += e.second;
    const uint64_t budget = c->em_many.batch_bytes ? c->em_many.batch_bytes : HML_EM_MANY_DEFAULT_BYTES;
    const uint64_t G0 = std::min<uint64_t>(std::max<uint64_t>(budget / member_bytes, 1u), R);
    for (const auto& e : layout) HIPCHK(e.first->alloc(G0 * e.second));
    {
        std::vector<hml_em_many_rec> recs(G0);
        for (uint64_t i = 0; i < G0; ++i) {
            hml_em_many_rec& r = recs[i];
            const uint64_t BK = (uint64_t)g.B * K, CK = (uint64_t)g.n_chunks * K;
            r.floats = b.floats.as<float>() + i * g.nfloats;
            r.mdl = b.mdl.as<hml_model>() + i;
            r.par = b.par.as<hml_vit_par>() + i;
            r.A = b.A.as<double>() + i * KK; r.pi = b.pi.as<double>() + i * K;
            r.match = b.match.as<uint8_t>() + i * g.n_chunks;
            r.heads = b.heads.as<uint32_t>() + i * g.n_chunks;
            r.cnt = b.cnt.as<uint32_t>() + 2 * i;
            r.words = b.words.as<unsigned long long>() + i * HML_EMM_WORDS;
            r.lt[0] = b.lt1.as<double>() + i * g.n1; r.lt[1] = b.lt2.as<double>() + i * g.n2;
            r.pt[0] = b.p1.as<double>() + i * g.n1 * g.ncols; r.pt[1] = b.p2.as<double>() + i * g.n2 * g.ncols;
            r.X = g.small ? nullptr : b.X.as<double>() + i * g.B;
            r.result = b.result.as<double>() + i * g.nresult;
            hml_post_args& f = r.dir[0];
            f = post_args_of(c, r.par, r.A, r.pi, g.L, g.W, g.n_chunks, b.entry.as<double>() + i * CK, b.exitv.as<double>() + i * CK);
            f.rows = b.alpha.as<double>() + i * BK; f.cval = b.cval.as<double>() + i * g.B; f.ell = b.ell.as<double>() + i * g.B;
            r.dir[1] = f;
            r.dir[1].rows = b.beta.as<double>() + i * BK; r.dir[1].cval = nullptr; r.dir[1].ell = nullptr;   // (entry, exit, match and heads are used again)
            hml_em_args& e = r.em;
            e.par = r.par; e.A = r.A; e.ia = c->d_ia; e.starts = c->d_starts.get();
            e.alpha = f.rows; e.beta = r.dir[1].rows; e.X = r.X; e.part = r.pt[0]; e.first = b.first.as<double>() + i * K;
        }
        HIPCHK(hipMemcpyAsync(b.recs.get(), recs.data(), G0 * sizeof(hml_em_many_rec), hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));   // (the records leave this frame)
    }

    // the members: their floats, the last two trace entries, and who still runs
    std::vector<float> mv(mean_var, mean_var + R * 2u * P), tA(A, A + R * (uint64_t)KK), tpi(pi, pi + R * (uint64_t)K);
    std::vector<double> prev(R, 0.0), cur(R, 0.0);
    std::vector<uint64_t> n_steps(R, 0), n_kept(R, 0);
    std::vector<int> why(R, HML_EM_MAX_STEPS);
    std::vector<uint64_t> active(R), next;
    for (uint64_t r = 0; r < R; ++r) active[r] = r;
    if (trace) std::fill(trace, trace + R * (max_steps + 1u), std::numeric_limits<double>::quiet_NaN());
    std::vector<float> h_floats(G0 * g.nfloats);
    std::vector<double> h_result(G0 * g.nresult);
    em_many_stats st;
    uint64_t esteps = 0, first_groups = 0;
    for (uint64_t k = 0; !active.empty(); ++k, ++esteps) {
        next.clear();
        const uint64_t G = std::min<uint64_t>(G0, active.size());
        if (k == 0) first_groups = (active.size() + G - 1u) / G;
        for (uint64_t off = 0; off < active.size(); off += G) {
            const uint32_t n = (uint32_t)std::min<uint64_t>(G, active.size() - off);
            for (uint32_t i = 0; i < n; ++i) {
                const uint64_t r = active[off + i];
                float* const f = h_floats.data() + i * g.nfloats;
                std::copy(mv.begin() + r * 2u * P, mv.begin() + (r + 1u) * 2u * P, f);
                std::copy(tA.begin() + r * KK, tA.begin() + (r + 1u) * KK, f + 2 * P);
                std::copy(tpi.begin() + r * K, tpi.begin() + (r + 1u) * K, f + 2 * P + KK);
            }
            if (int r = em_many_estep(c, g, b, n, h_floats.data(), h_result.data(), st)) return r;
            for (uint32_t i = 0; i < n; ++i) {
                const uint64_t r = active[off + i];
                hml_em_counts cnt;
                uint64_t walked = 0;
                em_many_counts(g, h_result.data() + i * g.nresult, cnt, &walked);
                st.walked += walked;
                float* const rmv = mv.data() + r * 2u * P;
                float* const rA = tA.data() + r * KK;
                float* const rpi = tpi.data() + r * K;
                prev[r] = cur[r];
                cur[r] = hml_em_objective(K, P, use_prior, q0.pr, cnt.loglik, rmv, rA, rpi);
                if (trace) trace[r * (max_steps + 1u) + k] = cur[r];
                if (hml_em_stops(prev[r], cur[r], k, max_steps, rel_tol, cnt.degenerate + cnt.xi_degenerate, &why[r])) { n_steps[r] = k; continue; }
                n_kept[r] += hml_em_mstep(K, g.D, P, q0.self_trans, use_prior, q0.pr, cnt, rmv, rA, rpi);
                next.push_back(r);
            }
        }
        active.swap(next);
    }
    const int64_t win = hml_em_many_best(R, why.data(), cur.data());
    if (install && win >= 0)
        if (int r = hml_set_parameters(c, mv.data() + (uint64_t)win * 2u * P, tA.data() + (uint64_t)win * KK, tpi.data() + (uint64_t)win * K)) return r;
    if (steps) std::copy(n_steps.begin(), n_steps.end(), steps);
    if (reason) std::copy(why.begin(), why.end(), reason);
    if (kept) std::copy(n_kept.begin(), n_kept.end(), kept);
    if (fit_mean_var) std::copy(mv.begin(), mv.end(), fit_mean_var);
    if (fit_A) std::copy(tA.begin(), tA.end(), fit_A);
    if (fit_pi) std::copy(tpi.begin(), tpi.end(), fit_pi);
    if (objective) std::copy(cur.begin(), cur.end(), objective);
    if (best) *best = win;
    c->em_many.computed = true;
    c->em_many.members = R; c->em_many.groups = first_groups; c->em_many.group_size = G0; c->em_many.esteps = esteps; c->em_many.launch_sets = st.launch_sets;
    c->em_many.stale_fwd = st.stale[0]; c->em_many.stale_bwd = st.stale[1]; c->em_many.rounds_run = st.rounds; c->em_many.walked = st.walked;
    return 0;
}

int hml_em_starts(hml_ctx* c, uint64_t R, uint64_t seed, double spread, float* mean_var, float* A, float* pi) {
    NEED_MODEL();
    if (R < 1u || R > HML_EM_MANY_MAX_R) return set_err(HML_ERR_ARG, "hml_em_starts: the number of members must be 1 ... " + std::to_string(HML_EM_MANY_MAX_R));
    if (!mean_var) return set_err(HML_ERR_ARG, "null argument");
    em_params q;
    if (int r = em_fetch(c, q)) return r;
    if (!hml_em_many_starts(c->K, q.P, R, seed, spread, q.mv.data(), q.A.data(), q.pi.data(), mean_var, A, pi))
        return set_err(HML_ERR_ARG, "hml_em_starts: spread must be finite and positive");
    return 0;
}

int hml_em_many_info(hml_ctx* c, uint64_t* members, uint64_t* groups, uint64_t* group_size, uint64_t* esteps, uint64_t* launch_sets, uint64_t* stale_fwd,
                     uint64_t* stale_bwd, uint64_t* rounds, uint64_t* serial_chunks) {
    if (!c) return set_err(HML_ERR_ARG, "null context");
    if (!c->em_many.computed) return set_err(HML_ERR_ARG, "hml_em_many_info: nothing was computed yet");
    if (members) *members = c->em_many.members;
    if (groups) *groups = c->em_many.groups;
    if (group_size) *group_size = c->em_many.group_size;
    if (esteps) *esteps = c->em_many.esteps;
    if (launch_sets) *launch_sets = c->em_many.launch_sets;
    if (stale_fwd) *stale_fwd = c->em_many.stale_fwd;
    if (stale_bwd) *stale_bwd = c->em_many.stale_bwd;
    if (rounds) *rounds = c->em_many.rounds_run;
    if (serial_chunks) *serial_chunks = c->em_many.walked;
    return 0;
}

int hml_set_em_batch_bytes(hml_ctx* c, uint64_t bytes) {
    if (!c) return set_err(HML_ERR_ARG, "null context");
    c->em_many.batch_bytes = bytes;
    return 0;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------- pairwise read-outs (hml_k_pairs.h)
// Breakpoint and region posteriors under the current parameters: exact functions of the rows alpha and beta a smoothing pass
// leaves behind.  The chain is only read; device memory is local to a call, as the smoothing's is.

struct pairs_result {
    post_result post;   // alpha and beta (c_b, the calls and their confidences are released)
    DevBuf col, p, r;   // [2 K + 1][B] words: the terms, then their inclusive prefix sums; p[B]; r[B][K] for the probe alone
    uint64_t bad = 0;
    uint32_t B = 0;
};

// a smoothing pass, then the terms per block; the prefix sums only if asked (the probe reads the terms themselves)
static int pairs_compute(hml_ctx* c, bool want_r, bool scan, pairs_result& out) {
    infer_tables t;
    if (int r = post_compute(c, false, out.post, t)) return r;
    out.post.cval.free(); out.post.conf.free(); out.post.q.free();
    const int K = c->K;
    const uint32_t B = out.post.B;
    const int rows = 2 * K + 1;
    DevBuf b_bad;
    HIPCHK(out.col.alloc((uint64_t)rows * B * sizeof(unsigned long long)));
    HIPCHK(out.p.alloc((uint64_t)B * sizeof(double)));
    if (want_r) HIPCHK(out.r.alloc((uint64_t)B * K * sizeof(double)));
    HIPCHK(b_bad.alloc(sizeof(unsigned long long)));
    HIPCHK(hipMemsetAsync(b_bad.get(), 0, sizeof(unsigned long long), c->stream));
    const hml_post_args a = post_args_of(c, t);
    by_states(K, [&](auto km) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_k_pair_terms<km()>), dim3((B + 63u) / 64u), dim3(64), ((size_t)K * K + K) * sizeof(double), c->stream, a, out.post.alpha.as<double>(),
                           out.post.beta.as<double>(), out.col.as<unsigned long long>(), out.p.as<double>(), out.r.as<double>(), b_bad.as<unsigned long long>());
    });
    KLAUNCH_CHECK();
    unsigned long long n_bad = 0;
    HIPCHK(hipMemcpyAsync(&n_bad, b_bad.get(), sizeof n_bad, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));   // (the tables go with this frame)
    if (scan)
        if (int r = scan_rows<unsigned long long, unsigned long long, false>(c->stream, out.col.as<unsigned long long>(), B, rows, out.col.as<unsigned long long>())) return r;
    out.bad = n_bad;
    out.B = B;
    return 0;
}

extern "C" {

int hml_posterior_breaks(hml_ctx* c, double min_prob, uint64_t* n, uint32_t* pos, double* prob, double* expected_breaks, uint64_t* pair_degenerate) {
    NEED_MODEL();
    if (!n) return set_err(HML_ERR_ARG, "null argument");
    if (min_prob != min_prob) return set_err(HML_ERR_ARG, "hml_posterior_breaks: min_prob is not a number");
    pairs_result pr;
    if (int r = pairs_compute(c, false, true, pr)) return r;
    const uint32_t B = pr.B;
    if (B > 0x7fffffffu) return set_err(HML_ERR_ARG, "hml_posterior_breaks: more than 2^31 - 1 blocks: the list's counts are 32-bit");
    const uint32_t n_chunks = (uint32_t)(((uint64_t)B + 255u) / 256u);
    DevBuf b_cnt, b_pos, b_prob;
    HIPCHK(b_cnt.alloc(((uint64_t)n_chunks + 1) * sizeof(int32_t)));
    int32_t* const d_cnt = b_cnt.as<int32_t>();
    HIPCHK(hipMemsetAsync(d_cnt + n_chunks, 0, sizeof(int32_t), c->stream));
    hipLaunchKernelGGL(hml_k_pair_break_count, dim3(n_chunks), dim3(256), 0, c->stream, pr.p.as<double>(), B, min_prob, d_cnt);
    hipLaunchKernelGGL(hml_k_scan_chunks<int32_t>, dim3(1), dim3(1024), 0, c->stream, d_cnt, n_chunks + 1u);   // d_cnt[n_chunks] = total
    KLAUNCH_CHECK();
    int32_t M = 0;
    unsigned long long units = 0;
    HIPCHK(hipMemcpyAsync(&M, d_cnt + n_chunks, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(&units, pr.col.as<unsigned long long>() + (B - 1u), sizeof units, hipMemcpyDeviceToHost, c->stream));   // N[B - 1]
    HIPCHK(hipStreamSynchronize(c->stream));
    *n = (uint64_t)M;
    if (expected_breaks) *expected_breaks = (double)units * (1.0 / 4294967296.0);
    if (pair_degenerate) *pair_degenerate = pr.bad;
    if (!pos || M == 0) return 0;
    HIPCHK(b_pos.alloc((uint64_t)M * sizeof(uint32_t)));
    HIPCHK(b_prob.alloc((uint64_t)M * sizeof(double)));
    hipLaunchKernelGGL(hml_k_pair_break_scatter, dim3(n_chunks), dim3(256), 0, c->stream, pr.p.as<double>(), c->d_starts.get(), B, min_prob, d_cnt, b_pos.as<uint32_t>(),
                       b_prob.as<double>());
    KLAUNCH_CHECK();
    HIPCHK(hipMemcpyAsync(pos, b_pos.get(), (uint64_t)M * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    if (prob) HIPCHK(hipMemcpyAsync(prob, b_prob.get(), (uint64_t)M * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

int hml_posterior_regions(hml_ctx* c, uint64_t n, const uint32_t* start, const uint32_t* end, double* whole, double* whole_state, double* expected_breaks, double* share,
                          uint64_t* raw, uint64_t* pair_degenerate) {
    NEED_MODEL();
    if (n && (!start || !end)) return set_err(HML_ERR_ARG, "null argument");
    for (uint64_t i = 0; i < n; ++i)
        if (!hml_pairs_region_ok(start[i], end[i], c->T)) {
            char buf[160];
            snprintf(buf, sizeof buf, "hml_posterior_regions: region %llu is [%u, %u): it must hold a position and end at or before T = %llu", (unsigned long long)i, start[i],
                     end[i], (unsigned long long)c->T);
            return set_err(HML_ERR_ARG, buf);
        }
    pairs_result pr;
    if (int r = pairs_compute(c, false, true, pr)) return r;
    if (pair_degenerate) *pair_degenerate = pr.bad;
    if (n == 0) return 0;
    const int K = c->K;
    const uint64_t nk = n * (uint64_t)K, nraw = n * (uint64_t)(2 * K + 1);
    DevBuf b_st, b_en, b_whole, b_ws, b_eb, b_share, b_raw;
    HIPCHK(b_st.alloc(n * sizeof(uint32_t)));
    HIPCHK(b_en.alloc(n * sizeof(uint32_t)));
    HIPCHK(b_whole.alloc(n * sizeof(double)));
    HIPCHK(b_ws.alloc(nk * sizeof(double)));
    HIPCHK(b_eb.alloc(n * sizeof(double)));
    HIPCHK(b_share.alloc(nk * sizeof(double)));
    HIPCHK(b_raw.alloc(nraw * sizeof(unsigned long long)));
    HIPCHK(hipMemcpyAsync(b_st.get(), start, n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(b_en.get(), end, n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    hml_pair_regions_out o;
    o.whole = b_whole.as<double>(); o.whole_state = b_ws.as<double>(); o.expected_breaks = b_eb.as<double>(); o.share = b_share.as<double>();
    o.raw = b_raw.as<unsigned long long>();
    hipLaunchKernelGGL(hml_k_pair_regions, dim3(grid_for(n, 256, 1, 4096)), dim3(256), 0, c->stream, c->d_starts.get(), pr.B, K, pr.post.alpha.as<double>(),
                       pr.post.beta.as<double>(), pr.col.as<unsigned long long>(), b_st.as<uint32_t>(), b_en.as<uint32_t>(), n, o);
    KLAUNCH_CHECK();
    if (whole) HIPCHK(hipMemcpyAsync(whole, b_whole.get(), n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (whole_state) HIPCHK(hipMemcpyAsync(whole_state, b_ws.get(), nk * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (expected_breaks) HIPCHK(hipMemcpyAsync(expected_breaks, b_eb.get(), n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (share) HIPCHK(hipMemcpyAsync(share, b_share.get(), nk * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (raw) HIPCHK(hipMemcpyAsync(raw, b_raw.get(), nraw * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));   // (the scratch goes with this frame)
    return 0;
}

int hml_posterior_pair_terms(hml_ctx* c, double* p, double* r, uint64_t* pfx, uint64_t* cost, uint64_t* mass) {
    NEED_MODEL();
    pairs_result pr;
    if (int rc = pairs_compute(c, r != nullptr, false, pr)) return rc;
    const int K = c->K;
    const uint64_t B = pr.B;
    std::vector<uint64_t> cols;
    if (cost || mass) cols.resize((uint64_t)(2 * K + 1) * B);
    if (p) HIPCHK(hipMemcpyAsync(p, pr.p.get(), B * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (r) HIPCHK(hipMemcpyAsync(r, pr.r.get(), B * K * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (pfx) HIPCHK(hipMemcpyAsync(pfx, pr.col.get(), B * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    if (!cols.empty()) HIPCHK(hipMemcpyAsync(cols.data(), pr.col.get(), cols.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (uint64_t b = 0; b < B && !cols.empty(); ++b)   // the columns, by block
        for (int j = 0; j < K; ++j) {
            if (cost) cost[b * K + j] = cols[(uint64_t)(1 + j) * B + b];
            if (mass) mass[b * K + j] = cols[(uint64_t)(1 + K + j) * B + b];
        }
    return 0;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------- sampled paths (hml_k_sample.h)
// Independent draws of whole paths from p(q | y, theta): the forward half of a smoothing pass, then the draws in groups of as
// many as the byte budget holds.  Every count is an integer sum that the groups add to, so no word depends on the grouping.
// The chain is only read; device memory is local to the call.
#define HML_SAMPLE_DEFAULT_BYTES (4ull << 30)   // of a group's device memory (hml_set_sample_batch_bytes)
#define HML_SAMPLE_MAX_COUNT (1ull << 24)
#define HML_SAMPLE_MAX_GROUP (1ull << 20)       // (grid dimension y of the first run: draws / 256)

struct sample_request {
    uint64_t first = 0, count = 0, seed = 0;
    uint8_t* paths = nullptr;
    uint64_t* segments = nullptr;
    int64_t* score_fixed = nullptr;
    uint32_t *change_count = nullptr, *state_count = nullptr;
    uint64_t* sample_degenerate = nullptr;
    uint64_t n_regions = 0;
    const uint32_t *start = nullptr, *end = nullptr;
    uint32_t H = 0;
    uint32_t *hist = nullptr, *whole_state = nullptr;
    uint64_t *breaks_sum = nullptr, *breaks_sq = nullptr;
};

static int sample_run(hml_ctx* c, const char* who, const sample_request& q) {
    if (q.count < 1u || q.count > HML_SAMPLE_MAX_COUNT) return set_err(HML_ERR_ARG, std::string(who) + ": count must be 1 ... 2^24");
    if (q.first > (1ull << 48) || q.first + q.count > (1ull << 48)) return set_err(HML_ERR_ARG, std::string(who) + ": first + count must not exceed 2^48");
    const int K = c->K;
    infer_tables t, ts;   // A and pi in double; the decode's fixed-point terms, for the scores
    post_result post;
    {
        post_forward_scratch s;
        if (int r = post_forward(c, post, t, s)) return r;
        HIPCHK(hipStreamSynchronize(c->stream));   // (the scratch goes with this frame)
    }
    post.cval.free();
    const uint32_t B = post.B;
    const chunk_geom cg = chunk_geom_of(c->samp, HML_SAMP_DEFAULT_L, HML_SAMP_DEFAULT_W, B);
    const uint32_t L = cg.L, W = cg.W, n_chunks = cg.n_chunks;
    const bool want_regions = q.n_regions != 0;
    const bool want_counts = q.change_count || q.state_count;

    // what lives for the whole call
    DevBuf b_guess, b_emit, b_cc, b_sc, b_st, b_en, b_hist, b_ws, b_bs, b_bq, b_words;
    HIPCHK(b_guess.alloc(B));
    hipLaunchKernelGGL(hml_k_samp_guess, dim3(grid_for(B, 256, 1, 16384)), dim3(256), 0, c->stream, post.alpha.as<double>(), K, B, b_guess.as<uint8_t>());
    KLAUNCH_CHECK();
    if (q.score_fixed) {
        uint32_t B2 = 0;
        if (int r = vit_begin(c, ts, &B2)) return r;
        HIPCHK(b_emit.alloc((uint64_t)B * K * sizeof(long long)));
        hipLaunchKernelGGL(hml_k_vit_emit_table, dim3(grid_for(B, 256, 1, 16384)), dim3(256), 0, c->stream, ts.par.as<hml_vit_par>(), c->d_ia, c->d_starts.get(), b_emit.as<long long>());
        KLAUNCH_CHECK();
    }
    if (want_counts) {
        HIPCHK(b_cc.alloc((uint64_t)B * sizeof(uint32_t)));
        HIPCHK(hipMemsetAsync(b_cc.get(), 0, (uint64_t)B * sizeof(uint32_t), c->stream));
        if (q.state_count) {
            HIPCHK(b_sc.alloc((uint64_t)B * K * sizeof(uint32_t)));
            HIPCHK(hipMemsetAsync(b_sc.get(), 0, (uint64_t)B * K * sizeof(uint32_t), c->stream));
        }
    }
    const uint64_t n = q.n_regions, nh = n * (q.H + 1ull), nk = n * (uint64_t)K;
    if (want_regions) {
        HIPCHK(b_st.alloc(n * sizeof(uint32_t)));
        HIPCHK(b_en.alloc(n * sizeof(uint32_t)));
        HIPCHK(b_hist.alloc(nh * sizeof(uint32_t)));
        HIPCHK(b_ws.alloc(nk * sizeof(uint32_t)));
        HIPCHK(b_bs.alloc(n * sizeof(unsigned long long)));
        HIPCHK(b_bq.alloc(n * sizeof(unsigned long long)));
        HIPCHK(hipMemcpyAsync(b_st.get(), q.start, n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(b_en.get(), q.end, n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemsetAsync(b_hist.get(), 0, nh * sizeof(uint32_t), c->stream));
        HIPCHK(hipMemsetAsync(b_ws.get(), 0, nk * sizeof(uint32_t), c->stream));
        HIPCHK(hipMemsetAsync(b_bs.get(), 0, n * sizeof(unsigned long long), c->stream));
        HIPCHK(hipMemsetAsync(b_bq.get(), 0, n * sizeof(unsigned long long), c->stream));
    }
    HIPCHK(b_words.alloc(4 * sizeof(unsigned long long)));   // [0] stale pairs and heads (32 bits each), [1] pairs the finishing lanes ran, [2] degenerate blocks
    unsigned long long* const words = b_words.as<unsigned long long>();
    HIPCHK(hipMemsetAsync(words, 0, 4 * sizeof(unsigned long long), c->stream));

    // the group: a draw's bytes are its path (twice if the caller takes the paths: the transposed copy), the words of its chunks
    // and its two sums; pair indices are 32-bit
    const uint64_t draw_bytes = (uint64_t)B * (q.paths ? 2u : 1u) + (uint64_t)n_chunks * (2u + 2u * sizeof(uint32_t)) + 2u * sizeof(unsigned long long);
    const uint64_t budget = c->samp_batch.batch_bytes ? c->samp_batch.batch_bytes : HML_SAMPLE_DEFAULT_BYTES;
    uint64_t G0 = std::max<uint64_t>(budget / draw_bytes, 1u);
    G0 = std::min<uint64_t>(G0, std::max<uint64_t>(0xffffffffull / n_chunks, 1u));
    G0 = std::min<uint64_t>(std::min<uint64_t>(G0, HML_SAMPLE_MAX_GROUP), q.count);
    const uint64_t pairs0 = G0 * n_chunks;
    DevBuf b_path, b_out, b_entry, b_exit, b_deg, b_list, b_chg, b_score;
    HIPCHK(b_path.alloc(G0 * B));
    if (q.paths) HIPCHK(b_out.alloc(G0 * B));
    HIPCHK(b_entry.alloc(pairs0));
    HIPCHK(b_exit.alloc(pairs0));
    HIPCHK(b_deg.alloc(pairs0 * sizeof(uint32_t)));
    HIPCHK(b_list.alloc(pairs0 * sizeof(uint32_t)));
    HIPCHK(b_chg.alloc(G0 * sizeof(unsigned long long)));
    HIPCHK(b_score.alloc(G0 * sizeof(unsigned long long)));

    hml_samp_args a;
    a.alpha = post.alpha.as<double>(); a.A = t.trans.as<double>(); a.guess = b_guess.as<uint8_t>();
    a.K = K; a.B = B; a.L = L; a.W = W; a.n_chunks = n_chunks; a.seed = q.seed;
    a.path = b_path.as<uint8_t>(); a.entry = b_entry.as<uint8_t>(); a.exitv = b_exit.as<uint8_t>(); a.deg = b_deg.as<uint32_t>();
    const size_t lds = (size_t)K * (K + 1) * sizeof(double);
    std::vector<unsigned long long> h_chg(G0), h_score(G0);
    uint64_t stale_first = 0, rounds_run = 0, n_groups = 0;
    for (uint64_t off = 0; off < q.count; off += G0, ++n_groups) {
        const uint32_t G = (uint32_t)std::min<uint64_t>(G0, q.count - off);
        const uint64_t n_pairs = (uint64_t)G * n_chunks;
        a.G = G; a.first = q.first + off;
        HIPCHK(hipMemsetAsync(b_entry.get(), 0, n_pairs, c->stream));
        HIPCHK(hipMemsetAsync(b_chg.get(), 0, (uint64_t)G * sizeof(unsigned long long), c->stream));
        HIPCHK(hipMemsetAsync(b_score.get(), 0, (uint64_t)G * sizeof(unsigned long long), c->stream));
        const dim3 grid(n_chunks, (G + HML_SAMP_LANES - 1u) / HML_SAMP_LANES);
        by_states(K, [&](auto km) { hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_k_samp_first<km()>), grid, dim3(HML_SAMP_LANES), lds, c->stream, a); });
        KLAUNCH_CHECK();
        auto verify = [&](uint64_t* stale, uint32_t* heads) {
            uint32_t h_cnt[2] = {0, 0};
            if (n_chunks > 1u) {
                HIPCHK(hipMemsetAsync(words, 0, sizeof h_cnt, c->stream));
                hipLaunchKernelGGL(hml_k_samp_verify, dim3(grid_for(n_pairs - G, 256, 1, 4096)), dim3(256), 0, c->stream, a.entry, a.exitv, G, n_pairs, b_list.as<uint32_t>(),
                                   (uint32_t*)words, (uint32_t*)words + 1);
                KLAUNCH_CHECK();
                HIPCHK(hipMemcpyAsync(h_cnt, words, sizeof h_cnt, hipMemcpyDeviceToHost, c->stream));
                HIPCHK(hipStreamSynchronize(c->stream));
            }
            *stale = h_cnt[0]; *heads = h_cnt[1];
            return 0;
        };
        auto rerun = [&](uint32_t n_heads) {
            by_states(K, [&](auto km) {
                hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_k_samp_rerun<km()>), dim3((n_heads + 63u) / 64u), dim3(64), lds, c->stream, a, b_list.as<uint32_t>(), n_heads);
            });
        };
        auto finish = [&] {
            by_states(K, [&](auto km) { hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_k_samp_finish<km()>), dim3((G + 63u) / 64u), dim3(64), lds, c->stream, a, words + 1); });
        };
        repair_outcome rep;
        if (int r = repair_rounds(c->samp.rounds, verify, rerun, finish, rep)) return r;
        stale_first += rep.stale_first;
        rounds_run = std::max(rounds_run, rep.rounds);

        // the paths of the group are final: what is read off them
        hipLaunchKernelGGL(hml_k_samp_deg_sum, dim3(grid_for(n_pairs, 256, 1, 4096)), dim3(256), 0, c->stream, a.deg, n_pairs, words + 2);
        if (q.segments || q.score_fixed)
            hipLaunchKernelGGL(hml_k_samp_draw_stats, grid, dim3(HML_SAMP_LANES), 0, c->stream, a, q.score_fixed ? b_emit.as<long long>() : nullptr, ts.trans.as<long long>(),
                               ts.init.as<long long>(), b_chg.as<unsigned long long>(), b_score.as<unsigned long long>());
        if (want_counts)
            hipLaunchKernelGGL(hml_k_samp_block_counts, dim3(grid_for(B, 1, 1, 65536)), dim3(64), 0, c->stream, a.path, K, B, G, b_cc.as<uint32_t>(), b_sc.as<uint32_t>());
        if (want_regions) {
            hml_samp_regions_out o;
            o.hist = b_hist.as<uint32_t>(); o.whole_state = b_ws.as<uint32_t>(); o.breaks_sum = b_bs.as<unsigned long long>(); o.breaks_sq = b_bq.as<unsigned long long>();
            hipLaunchKernelGGL(hml_k_samp_regions, dim3((G + 255u) / 256u, (unsigned)std::min<uint64_t>(n, 65535u)), dim3(256), 0, c->stream, a.path, c->d_starts.get(), K, B, G,
                               b_st.as<uint32_t>(), b_en.as<uint32_t>(), n, q.H, o);
        }
        if (q.paths) hipLaunchKernelGGL(hml_k_samp_transpose, dim3((B + 63u) / 64u, (G + 63u) / 64u), dim3(256), 0, c->stream, a.path, B, G, b_out.as<uint8_t>());
        KLAUNCH_CHECK();
        if (q.paths) HIPCHK(hipMemcpyAsync(q.paths + off * B, b_out.get(), (uint64_t)G * B, hipMemcpyDeviceToHost, c->stream));
        if (q.segments) HIPCHK(hipMemcpyAsync(h_chg.data(), b_chg.get(), (uint64_t)G * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
        if (q.score_fixed) HIPCHK(hipMemcpyAsync(h_score.data(), b_score.get(), (uint64_t)G * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        for (uint32_t g = 0; g < G; ++g) {
            if (q.segments) q.segments[off + g] = 1u + h_chg[g];
            if (q.score_fixed) q.score_fixed[off + g] = (int64_t)h_score[g];
        }
    }
    unsigned long long h_words[4];
    HIPCHK(hipMemcpyAsync(h_words, words, sizeof h_words, hipMemcpyDeviceToHost, c->stream));
    if (q.change_count) HIPCHK(hipMemcpyAsync(q.change_count, b_cc.get(), (uint64_t)B * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    if (q.state_count) HIPCHK(hipMemcpyAsync(q.state_count, b_sc.get(), (uint64_t)B * K * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    if (want_regions) {
        if (q.hist) HIPCHK(hipMemcpyAsync(q.hist, b_hist.get(), nh * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        if (q.whole_state) HIPCHK(hipMemcpyAsync(q.whole_state, b_ws.get(), nk * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        if (q.breaks_sum) HIPCHK(hipMemcpyAsync(q.breaks_sum, b_bs.get(), n * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
        if (q.breaks_sq) HIPCHK(hipMemcpyAsync(q.breaks_sq, b_bq.get(), n * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(hipStreamSynchronize(c->stream));   // (the scratch goes with this frame)
    if (q.sample_degenerate) *q.sample_degenerate = h_words[2];
    c->samp.done = true;
    c->samp.chunks = n_chunks; c->samp.used_L = L; c->samp.used_W = W; c->samp.stale[0] = stale_first; c->samp.rounds_run = rounds_run; c->samp.walked = h_words[1];
    c->samp_batch.draws = q.count; c->samp_batch.groups = n_groups; c->samp_batch.group_size = G0;
    return 0;
}

extern "C" {

int hml_posterior_sample(hml_ctx* c, uint64_t first, uint64_t count, uint64_t seed, uint8_t* paths, uint64_t* segments, int64_t* score_fixed, uint32_t* change_count,
                         uint32_t* state_count, uint64_t* sample_degenerate) {
    NEED_MODEL();
    sample_request q;
    q.first = first; q.count = count; q.seed = seed;
    q.paths = paths; q.segments = segments; q.score_fixed = score_fixed; q.change_count = change_count; q.state_count = state_count;
    q.sample_degenerate = sample_degenerate;
    return sample_run(c, "hml_posterior_sample", q);
}

int hml_posterior_sample_regions(hml_ctx* c, uint64_t first, uint64_t count, uint64_t seed, uint64_t n, const uint32_t* start, const uint32_t* end, uint32_t max_breaks,
                                 uint32_t* hist, uint32_t* whole_state, uint64_t* breaks_sum, uint64_t* breaks_sq) {
    NEED_MODEL();
    if (n && (!start || !end)) return set_err(HML_ERR_ARG, "null argument");
    if (max_breaks < 1u) return set_err(HML_ERR_ARG, "hml_posterior_sample_regions: max_breaks must be at least 1");
    for (uint64_t i = 0; i < n; ++i)
        if (!hml_pairs_region_ok(start[i], end[i], c->T)) {
            char buf[176];
            snprintf(buf, sizeof buf, "hml_posterior_sample_regions: region %llu is [%u, %u): it must hold a position and end at or before T = %llu", (unsigned long long)i,
                     start[i], end[i], (unsigned long long)c->T);
            return set_err(HML_ERR_ARG, buf);
        }
    sample_request q;
    q.first = first; q.count = count; q.seed = seed;
    q.n_regions = n; q.start = start; q.end = end; q.H = max_breaks;
    q.hist = hist; q.whole_state = whole_state; q.breaks_sum = breaks_sum; q.breaks_sq = breaks_sq;
    return sample_run(c, "hml_posterior_sample_regions", q);
}

int hml_posterior_sample_info(hml_ctx* c, uint64_t* draws, uint64_t* groups, uint64_t* group_size, uint64_t* chunks, uint64_t* L, uint64_t* W, uint64_t* stale_first,
                              uint64_t* rounds, uint64_t* serial_chunks) {
    if (!c) return set_err(HML_ERR_ARG, "null context");
    if (!c->samp.done) return set_err(HML_ERR_ARG, "hml_posterior_sample_info: nothing was sampled yet");
    if (draws) *draws = c->samp_batch.draws;
    if (groups) *groups = c->samp_batch.groups;
    if (group_size) *group_size = c->samp_batch.group_size;
    if (chunks) *chunks = c->samp.chunks;
    if (L) *L = c->samp.used_L;
    if (W) *W = c->samp.used_W;
    if (stale_first) *stale_first = c->samp.stale[0];
    if (rounds) *rounds = c->samp.rounds_run;
    if (serial_chunks) *serial_chunks = c->samp.walked;
    return 0;
}

int hml_set_sample_batch_bytes(hml_ctx* c, uint64_t bytes) {
    if (!c) return set_err(HML_ERR_ARG, "null context");
    c->samp_batch.batch_bytes = bytes;
    return 0;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------- count read-outs (hml_k_counts.h)
// Per region the exact distribution of the number of breakpoints and the probability of avoiding each state: forward
// recursions over the region's blocks on the posterior's own transitions, whose terms v_b and rho_b follow from the row beta a
// smoothing pass leaves behind.  The chain is only read; device memory is local to a call, as the smoothing's is.

struct counts_result {
    post_result post;   // alpha and beta (c_b, the calls and their confidences are released)
    infer_tables t;     // A and pi in double: the walks stage them as the terms kernel does
    DevBuf v, rho;      // [B][K] each
    uint64_t bad = 0;
    uint32_t B = 0;
};

// f(std::integral_constant<int, NC>()) for the cells a lane of a walk holds at the most
template <class F>
static void by_lane_cells(int cells, F f) {
    switch (hml_counts_lane_cells(cells)) {
        case 1: f(std::integral_constant<int, 1>()); break;
        case 2: f(std::integral_constant<int, 2>()); break;
        case 4: f(std::integral_constant<int, 4>()); break;
        case 8: f(std::integral_constant<int, 8>()); break;
        default: f(std::integral_constant<int, (int)HML_COUNTS_LANE_CELLS>()); break;
    }
}

// a smoothing pass, then the terms per block
static int counts_compute(hml_ctx* c, counts_result& out) {
    if (int r = post_compute(c, false, out.post, out.t)) return r;
    out.post.cval.free(); out.post.conf.free(); out.post.q.free();
    const int K = c->K;
    const uint32_t B = out.post.B;
    DevBuf b_bad;
    HIPCHK(out.v.alloc((uint64_t)B * K * sizeof(double)));
    HIPCHK(out.rho.alloc((uint64_t)B * K * sizeof(double)));
    HIPCHK(b_bad.alloc(sizeof(unsigned long long)));
    HIPCHK(hipMemsetAsync(b_bad.get(), 0, sizeof(unsigned long long), c->stream));
    const hml_post_args a = post_args_of(c, out.t);
    by_states(K, [&](auto km) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_k_count_terms<km()>), dim3((B + 63u) / 64u), dim3(64), ((size_t)K * K + K) * sizeof(double), c->stream, a,
                           out.post.beta.as<double>(), out.v.as<double>(), out.rho.as<double>(), b_bad.as<unsigned long long>());
    });
    KLAUNCH_CHECK();
    unsigned long long n_bad = 0;
    HIPCHK(hipMemcpyAsync(&n_bad, b_bad.get(), sizeof n_bad, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    out.bad = n_bad;
    out.B = B;
    return 0;
}

extern "C" {

int hml_posterior_region_counts(hml_ctx* c, uint64_t n, const uint32_t* start, const uint32_t* end, uint32_t max_breaks, double* hist, double* whole_state, double* avoid,
                                uint64_t* count_degenerate) {
    NEED_MODEL();
    if (n && (!start || !end)) return set_err(HML_ERR_ARG, "null argument");
    const int K = c->K;
    if (!hml_counts_h_ok(K, max_breaks)) {
        char buf[176];
        snprintf(buf, sizeof buf, "hml_posterior_region_counts: " HML_COUNTS_H_RULE " (K = %d, max_breaks = %u)", K, max_breaks);
        return set_err(HML_ERR_ARG, buf);
    }
    for (uint64_t i = 0; i < n; ++i)
        if (!hml_pairs_region_ok(start[i], end[i], c->T)) {
            char buf[176];
            snprintf(buf, sizeof buf, "hml_posterior_region_counts: region %llu is [%u, %u): it must hold a position and end at or before T = %llu", (unsigned long long)i,
                     start[i], end[i], (unsigned long long)c->T);
            return set_err(HML_ERR_ARG, buf);
        }
    counts_result cr;
    if (int r = counts_compute(c, cr)) return r;
    unsigned long long h_info[2] = {0ull, 0ull};
    if (n) {
        const uint32_t H = max_breaks;
        const uint64_t nh = n * (uint64_t)(H + 1u), nk = n * (uint64_t)K;
        DevBuf b_st, b_en, b_hist, b_ws, b_av, b_info;
        HIPCHK(b_st.alloc(n * sizeof(uint32_t)));
        HIPCHK(b_en.alloc(n * sizeof(uint32_t)));
        HIPCHK(b_hist.alloc(nh * sizeof(double)));
        HIPCHK(b_ws.alloc(nk * sizeof(double)));
        HIPCHK(b_av.alloc(nk * sizeof(double)));
        HIPCHK(b_info.alloc(sizeof h_info));
        HIPCHK(hipMemcpyAsync(b_st.get(), start, n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(b_en.get(), end, n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemsetAsync(b_info.get(), 0, sizeof h_info, c->stream));
        const hml_post_args a = post_args_of(c, cr.t);
        hml_count_walk_args w;
        w.alpha = cr.post.alpha.as<double>(); w.beta = cr.post.beta.as<double>(); w.v = cr.v.as<double>(); w.rho = cr.rho.as<double>();
        w.rg_start = b_st.as<uint32_t>(); w.rg_end = b_en.as<uint32_t>(); w.n = n; w.H = H;
        w.hist = b_hist.as<double>(); w.whole_state = b_ws.as<double>(); w.avoid = b_av.as<double>(); w.info = b_info.as<unsigned long long>();
        const size_t staged = ((size_t)K * K + 3u * K) * sizeof(double);   // A, pi, v_b, rho_b
        const unsigned grid = (unsigned)grid_for(n, 1, 1, 4096), slices = (unsigned)((K + HML_COUNTS_SLICE - 1) / HML_COUNTS_SLICE);
        const int slice_states = K < HML_COUNTS_SLICE ? K : HML_COUNTS_SLICE;
        by_lane_cells(K * (int)(H + 1u), [&](auto nc) {
            hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_k_count_walk<nc()>), dim3(grid), dim3(64), staged + (size_t)K * (H + 1u) * sizeof(double), c->stream, a, w);
        });
        by_lane_cells(K * slice_states, [&](auto nc) {
            hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_k_count_avoid<nc()>), dim3(grid, slices), dim3(64), staged + (size_t)K * slice_states * sizeof(double), c->stream, a, w);
        });
        KLAUNCH_CHECK();
        if (hist) HIPCHK(hipMemcpyAsync(hist, b_hist.get(), nh * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        if (whole_state) HIPCHK(hipMemcpyAsync(whole_state, b_ws.get(), nk * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        if (avoid) HIPCHK(hipMemcpyAsync(avoid, b_av.get(), nk * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(h_info, b_info.get(), sizeof h_info, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));   // (the scratch goes with this frame)
    }
    if (count_degenerate) *count_degenerate = cr.bad;
    c->counts.done = true;
    c->counts.regions = n; c->counts.steps = h_info[0]; c->counts.longest = h_info[1];
    return 0;
}

int hml_posterior_count_terms(hml_ctx* c, double* v, double* rho) {
    NEED_MODEL();
    counts_result cr;
    if (int r = counts_compute(c, cr)) return r;
    const uint64_t words = (uint64_t)cr.B * c->K;
    if (v) HIPCHK(hipMemcpyAsync(v, cr.v.get(), words * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (rho) HIPCHK(hipMemcpyAsync(rho, cr.rho.get(), words * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

int hml_posterior_counts_info(hml_ctx* c, uint64_t* regions, uint64_t* steps, uint64_t* longest) {
    if (!c) return set_err(HML_ERR_ARG, "null context");
    if (!c->counts.done) return set_err(HML_ERR_ARG, "hml_posterior_counts_info: nothing was computed yet");
    if (regions) *regions = c->counts.regions;
    if (steps) *steps = c->counts.steps;
    if (longest) *longest = c->counts.longest;
    return 0;
}

}  // extern "C"

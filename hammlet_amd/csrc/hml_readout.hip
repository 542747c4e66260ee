// libhammlet_hip.so - the read-outs of the C ABI (include/hml.h): what the recorded sweeps accumulated per position - state
// marginals, emission levels, breakpoints, level bands - brought into the forms the callers ask for, and the merges of one
// chain's recording into another's: on one device from recorder to recorder, across devices through the sparse payload of
// hml_k_rec_payload.h - and the chain's history.  Nothing here runs inside a sweep; hml_capi.hip holds the chain itself, and
// hml_infer.hip what is computed exactly under the current parameters and reads nothing a recorder wrote (Viterbi, smoothing, EM).
#define HML_REGIONS_KERNELS   // (hml_k_regions.h: this object holds the regions' kernels)
#include "hml_readout_shared.hpp"   // (the helpers hml_infer.hip needs too; it brings hml_capi_shared.hpp)
#include "hml_k_agree.h"   // (launched from this object alone)
#include "hml_k_rec_payload.h"

// The positions whose bit is set in a boundary bitmap over T positions (n_spans spans of HML_SPAN), ascending, on stream `s`:
// d_seg[M + 1] is allocated here, position 0 is always the first entry.  Counts per span, their prefix sums on the host, scatter.
static int compact_boundaries(hipStream_t s, const uint32_t* d_boundary, uint32_t T, uint32_t n_spans, uint64_t* M_out, DevBuf& d_seg) {
    DevBuf d_cnt, d_off;
    HIPCHK(d_cnt.alloc(n_spans * sizeof(uint32_t)));
    HIPCHK(d_off.alloc(n_spans * sizeof(uint32_t)));
    hipLaunchKernelGGL(hml_k_marg_count, dim3((n_spans + 3) / 4), dim3(256), 0, s, d_boundary, T, d_cnt.as<uint32_t>());
    std::vector<uint32_t> h_cnt(n_spans), h_off(n_spans);
    HIPCHK(hipMemcpyAsync(h_cnt.data(), d_cnt.get(), n_spans * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    uint64_t M = 0;
    for (uint32_t i = 0; i < n_spans; ++i) { h_off[i] = (uint32_t)M; M += h_cnt[i]; }
    HIPCHK(hipMemcpyAsync(d_off.get(), h_off.data(), n_spans * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    HIPCHK(d_seg.alloc((M + 1) * sizeof(uint32_t)));
    hipLaunchKernelGGL(hml_k_marg_scatter, dim3((n_spans + 3) / 4), dim3(256), 0, s, d_boundary, T, d_off.as<uint32_t>(), d_seg.as<uint32_t>());
    KLAUNCH_CHECK();
    HIPCHK(hipStreamSynchronize(s));   // (d_cnt and d_off go with this frame)
    *M_out = M;
    return 0;
}

// ---------------------------------------------------------------------------------------- count tables
// What the state marginals and the level bands both are: int32 difference rows [ncol][T + 1], touched only where a run starts,
// and the bitmap of those positions.  Read out as run-length segments (table_segments, table_rle), as a dense table
// (table_dense) and as runs of a per-segment key (table_runs).
struct hml_count_table {
    const int32_t* d_diff;
    const uint32_t* d_boundary;
    int ncol;
};
static hml_count_table marginal_table(const hml_ctx* c) { return {c->d_diff, c->d_boundary, c->K}; }
static hml_count_table band_table(const hml_ctx* c) {
    const hml_recorder& rec = c->rec[HML_REC_BANDS];
    return {rec.acc<int32_t>(), rec.d_boundary, recorder_rows(c, HML_REC_BANDS)};
}

// the table's segments on the device: starts d_seg[M] and the count differences at the starts d_g[M][ncol] (segment-major,
// hml_k_marg_gather)
static int table_segments(hml_ctx* c, const hml_count_table& tab, uint64_t* M_out, DevBuf& d_seg, DevBuf& d_g) {
    const uint32_t T = (uint32_t)c->T;
    uint64_t M = 0;
    if (int r = compact_boundaries(c->stream, tab.d_boundary, T, c->n_spans, &M, d_seg)) return r;
    HIPCHK(d_g.alloc(std::max<uint64_t>(M, 1) * tab.ncol * sizeof(int32_t)));
    hipLaunchKernelGGL(hml_k_marg_gather, dim3(grid_for(M, 256, 1, 16384)), dim3(256), 0, c->stream, tab.d_diff, T, tab.ncol, d_seg.as<uint32_t>(), (uint32_t)M, d_g.as<int32_t>());
    KLAUNCH_CHECK();
    HIPCHK(hipStreamSynchronize(c->stream));
    *M_out = M;
    return 0;
}

int hml_ctx_gather_marginal_segments(hml_ctx* c, uint64_t* M, DevBuf& d_seg, DevBuf& d_g) { return table_segments(c, marginal_table(c), M, d_seg, d_g); }

// the segments on the host: their lengths and, in counts[M][ncol_out], the counts of the first ncol_out columns - the running
// sums of the differences at all boundaries up to the segment
static int table_rle(hml_ctx* c, const hml_count_table& tab, uint64_t M, const DevBuf& d_seg, const DevBuf& d_g, int ncol_out, uint64_t* seg_len, int32_t* counts) {
    const int ncol = tab.ncol;
    std::vector<uint32_t> h_seg(M);
    std::vector<int32_t> h_g(M * ncol);
    HIPCHK(hipMemcpyAsync(h_seg.data(), d_seg.get(), M * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(h_g.data(), d_g.get(), M * ncol * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    lengths_of(h_seg.data(), M, (uint32_t)c->T, seg_len);
    if (!counts) return 0;
    std::vector<int32_t> cur(ncol_out, 0);
    for (uint64_t i = 0; i < M; ++i)
        for (int s = 0; s < ncol_out; ++s) counts[i * ncol_out + s] = cur[s] += h_g[i * ncol + s];
    return 0;
}

// the dense table out[ncol][T] on the device, enqueued on the context's stream: row j holds the prefix sums of difference row
// d_perm[j] (row j without a permutation).  d_cs: the scan's work array, the caller's until the stream is idle.
static int table_dense(hml_ctx* c, const hml_count_table& tab, const int32_t* d_perm, int32_t* out, DevBuf& d_cs) {
    const uint32_t T = (uint32_t)c->T;
    const uint32_t n_chunks = c->n_spans;
    HIPCHK(d_cs.alloc((uint64_t)tab.ncol * n_chunks * sizeof(int32_t)));
    hipLaunchKernelGGL(hml_k_dense_partial, dim3(n_chunks, tab.ncol), dim3(256), 0, c->stream, tab.d_diff, T, tab.ncol, d_cs.as<int32_t>(), n_chunks);
    hipLaunchKernelGGL(hml_k_scan_chunks<int32_t>, dim3(tab.ncol), dim3(1024), 0, c->stream, d_cs.as<int32_t>(), n_chunks);
    hipLaunchKernelGGL(hml_k_dense_final, dim3(n_chunks, tab.ncol), dim3(256), 0, c->stream, tab.d_diff, T, tab.ncol, d_cs.as<int32_t>(), n_chunks, d_perm, out);
    return 0;
}

// A 16-bit key per segment, adjacent segments with the same key merged into runs: *n_runs and, if run_len is given, the runs'
// lengths and keys.  pick(d_g, M, d_cs, n_chunks, d_key) launches the kernel that writes the keys from the differences d_g[M][ncol]
// and the exclusive sums d_cs[ncol][n_chunks] of their chunks of 256 segments (hml_k_segment.h).
template <class Pick>
static int table_runs(hml_ctx* c, const hml_count_table& tab, Pick pick, uint64_t* n_runs, uint64_t* run_len, std::vector<int16_t>& run_key) {
    const int ncol = tab.ncol;
    uint64_t M = 0;
    DevBuf b_seg, b_g, b_cs, b_key;
    if (int r = table_segments(c, tab, &M, b_seg, b_g)) return r;
    const uint32_t n_chunks = (uint32_t)((M + 255) / 256);
    HIPCHK(b_cs.alloc((uint64_t)ncol * n_chunks * sizeof(int32_t)));
    HIPCHK(b_key.alloc(M * sizeof(int16_t)));
    int32_t* const d_cs = b_cs.as<int32_t>();
    int16_t* const d_key = b_key.as<int16_t>();
    hipLaunchKernelGGL(hml_k_seg_partial, dim3(n_chunks), dim3(256), 0, c->stream, b_g.as<int32_t>(), (uint32_t)M, ncol, d_cs, n_chunks);
    hipLaunchKernelGGL(hml_k_scan_chunks<int32_t>, dim3(ncol), dim3(1024), 0, c->stream, d_cs, n_chunks);
    pick(b_g.as<int32_t>(), (uint32_t)M, d_cs, n_chunks, d_key);
    auto scatter = [&](uint32_t n_run_chunks, const int32_t* d_rc, uint64_t, uint32_t* d_rs, int16_t* d_rq) {
        hipLaunchKernelGGL(hml_k_seg_run_scatter, dim3(n_run_chunks), dim3(256), 0, c->stream, d_key, b_seg.as<uint32_t>(), (uint32_t)M, d_rc, d_rs, d_rq);
        return 0;
    };
    return merge_runs(c->stream, d_key, (uint32_t)M, (uint32_t)c->T, scatter, n_runs, run_len, run_key);
}

extern "C" {

// ---------------------------------------------------------------------------------------- state marginals
int hml_marginals_rle(hml_ctx* c, uint64_t* n_segments, int* n_columns, uint64_t* seg_len, int32_t* counts) {
    NEED_MODEL();
    hml_model m; if (int r = fetch_model(c, &m)) return r;
    if (int r = model_fault(m)) return r;
    const int ncol = m.max_state_recorded + 1;
    if (!c->d_diff || m.n_recorded == 0) {   // nothing recorded: one segment, no count columns
        *n_segments = 1; *n_columns = 0;
        if (seg_len) seg_len[0] = (uint32_t)c->T;
        return 0;
    }
    uint64_t M = 0;
    DevBuf b_seg, b_g;
    if (int r = table_segments(c, marginal_table(c), &M, b_seg, b_g)) return r;
    *n_segments = M; *n_columns = ncol;
    if (!seg_len) return 0;
    return table_rle(c, marginal_table(c), M, b_seg, b_g, ncol, seg_len, counts);
}

int hml_max_segmentation(hml_ctx* c, uint64_t* n_runs, uint64_t* run_len, int32_t* run_state) {
    NEED_MODEL();
    if (!n_runs) return set_err(HML_ERR_ARG, "null argument");
    hml_model m; if (int r = fetch_model(c, &m)) return r;
    if (int r = model_fault(m)) return r;
    const int K = c->K;
    if (!c->d_diff || m.n_recorded == 0) {   // nothing recorded: every count is zero, the arg-max is state 0
        *n_runs = 1;
        if (run_len) run_len[0] = (uint32_t)c->T;
        if (run_state) run_state[0] = 0;
        return 0;
    }
    std::vector<int16_t> state;
    auto argmax = [&](const int32_t* d_g, uint32_t M, const int32_t* d_cs, uint32_t n_chunks, int16_t* d_st) {
        if (K <= HML_MAX_K) hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_k_seg_argmax<HML_MAX_K>), dim3(n_chunks), dim3(256), 0, c->stream, d_g, M, K, d_cs, n_chunks, d_st);
        else hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_k_seg_argmax<HML_CAP_K>), dim3(n_chunks), dim3(256), 0, c->stream, d_g, M, K, d_cs, n_chunks, d_st);
    };
    if (int r = table_runs(c, marginal_table(c), argmax, n_runs, run_len, state)) return r;
    if (run_len && run_state) std::copy(state.begin(), state.end(), run_state);
    return 0;
}

int hml_marginals_dense_device(hml_ctx* c, void* out_dev, const int32_t* perm) {
    NEED_MODEL();
    const uint32_t T = (uint32_t)c->T;
    const int K = c->K;
    int32_t* out = (int32_t*)out_dev;
    if (!c->d_diff) {
        HIPCHK(hipMemsetAsync(out, 0, (uint64_t)(K + 1) * T * sizeof(int32_t), c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        return 0;
    }
    DevBuf b_cs, b_perm;
    if (perm) {
        uint64_t seen = 0u;
        for (int k = 0; k < K; ++k) {
            if (perm[k] < 0 || perm[k] >= K || ((seen >> perm[k]) & 1u)) return set_err(HML_ERR_ARG, "perm is not a permutation of the K states");
            seen |= (uint64_t)1 << perm[k];
        }
        HIPCHK(b_perm.alloc(K * sizeof(int32_t)));
        HIPCHK(hipMemcpyAsync(b_perm.get(), perm, K * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    }
    if (int r = table_dense(c, marginal_table(c), b_perm.as<int32_t>(), out, b_cs)) return r;
    hipLaunchKernelGGL(hml_k_dense_boundary, dim3(grid_for(T, 256, 1, 65536)), dim3(256), 0, c->stream, c->d_boundary, T,
                       out + (uint64_t)K * T);
    KLAUNCH_CHECK();
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------- emission levels (hml_k_levels.h)

// a recording's read-out may begin: it was asked for, its buffers exist (asked for, but no sweep was recorded yet: the empty
// answer of its kind, hml_ctx.hpp), the model is fetched and carries no device error
static int recorder_ready(hml_ctx* c, int kind, hml_model* m) {
    if (!c->rec[kind].asked) return recorder_none(kind, "this");
    if (int r = ensure_recorder_buffers(c, kind)) return r;
    if (int r = fetch_model(c, m)) return r;
    return model_fault(*m);
}

// hml_levels_merge / hml_breaks_merge / hml_bands_merge: the source's cells at the source's boundaries into the destination,
// on the destination's stream
static int recorder_merge(hml_ctx* dst, hml_ctx* src, int kind) {
    const hml_recorder_kind& rk = hml_recorder_kinds[kind];
    const bool per_dimension = kind != HML_REC_BREAKS;
    if (!dst || !src || !dst->model_set || !src->model_set) return set_err(HML_ERR_ARG, "model not set");
    if (dst == src) return set_err(HML_ERR_ARG, "a context cannot be merged into itself");
    if (dst->device != src->device)
        return set_err(HML_ERR_ARG, std::string("the ") + rk.noun + " of chains on different GPUs are not merged yet: run the chains of one " + rk.file + " file on one GPU");
    if (dst->T != src->T || (per_dimension && dst->D != src->D))
        return set_err(HML_ERR_ARG, std::string(rk.noun) + " can only be merged between chains over the same positions" + (per_dimension ? " and dimensions" : ""));
    if (!src->rec[kind].asked) return recorder_none(kind, "the source");
    if (kind == HML_REC_BANDS && !same_band_edges(dst, src->n_band_edges, src->band_edges)) {
        // a destination that was never asked takes the source's edges; any other difference is refused
        if (dst->rec[kind].asked || dst->rec[kind].d_acc) return set_err(HML_ERR_ARG, "level bands can only be merged between chains with the same edges, bit for bit");
        dst->n_band_edges = src->n_band_edges;
        memcpy(dst->band_edges, src->band_edges, sizeof dst->band_edges);
    }
    if (int r = ctx_bind(dst)) return r;
    if (int r = hml_settle(src)) return r;   // (both streams idle: the merge reads the source's accumulators on the destination's stream)
    if (int r = hml_settle(dst)) return r;
    if (int r = ensure_recorder_buffers(src, kind)) return r;
    if (int r = ensure_recorder_buffers(dst, kind)) return r;
    dst->rec[kind].asked = true;
    const hml_recorder &rs = src->rec[kind], &rd = dst->rec[kind];
    const uint32_t T = (uint32_t)src->T;
    const int rows = recorder_rows(src, kind);
    uint64_t M = 0;
    DevBuf b_seg;
    if (int r = compact_boundaries(dst->stream, rs.d_boundary, T, src->n_spans, &M, b_seg)) return r;
    const uint32_t* d_pos = b_seg.as<uint32_t>();
    if (kind == HML_REC_BREAKS) { ++d_pos; --M; }   // (position 0 is never a breakpoint; M = 0 still adds the source's count of recorded sweeps)
    const dim3 grid(grid_for(M, 256, 1, 16384));
    unsigned long long *const src_n = recorder_counter(src, kind), *const dst_n = recorder_counter(dst, kind);
    if (kind == HML_REC_LEVELS)
        hipLaunchKernelGGL(hml_k_rec_merge<double>, grid, dim3(256), 0, dst->stream, rs.acc<double>(), d_pos, (uint32_t)M, T, rows, src_n, rd.acc<double>(), rd.d_boundary, dst_n);
    else if (kind == HML_REC_BREAKS)
        hipLaunchKernelGGL(hml_k_rec_merge<uint32_t>, grid, dim3(256), 0, dst->stream, rs.acc<uint32_t>(), d_pos, (uint32_t)M, T, rows, src_n, rd.acc<uint32_t>(), rd.d_boundary, dst_n);
    else
        hipLaunchKernelGGL(hml_k_rec_merge<int32_t>, grid, dim3(256), 0, dst->stream, rs.acc<int32_t>(), d_pos, (uint32_t)M, T, rows, src_n, rd.acc<int32_t>(), rd.d_boundary, dst_n);
    KLAUNCH_CHECK();
    HIPCHK(hipStreamSynchronize(dst->stream));
    return 0;
}

// the levels' segments on the device: starts d_seg[M] and, per row, the inclusive sums over the segments d_sum[2 D][M]
static int gather_level_segments(hml_ctx* c, uint64_t* M_out, DevBuf& d_seg, DevBuf& d_sum) {
    const uint32_t T = (uint32_t)c->T;
    const int rows = 2 * c->D;
    const hml_recorder& rec = c->rec[HML_REC_LEVELS];
    uint64_t M = 0;
    if (int r = compact_boundaries(c->stream, rec.d_boundary, T, c->n_spans, &M, d_seg)) return r;
    HIPCHK(d_sum.alloc(M * rows * sizeof(double)));
    hipLaunchKernelGGL(hml_k_rec_gather<double>, dim3(grid_for(M, 256, 1, 16384)), dim3(256), 0, c->stream, rec.acc<double>(), T, rows, d_seg.as<uint32_t>(), (uint32_t)M, d_sum.as<double>());
    if (int r = scan_rows<double, double, false>(c->stream, d_sum.as<double>(), M, rows, d_sum.as<double>())) return r;
    *M_out = M;
    return 0;
}

extern "C" {

int hml_levels_rle(hml_ctx* c, uint64_t* n_segments, uint64_t* n_recorded, uint64_t* seg_len, double* sum, double* sum_sq) {
    NEED_MODEL();
    if (!n_segments) return set_err(HML_ERR_ARG, "null argument");
    hml_model m; if (int r = recorder_ready(c, HML_REC_LEVELS, &m)) return r;
    const uint32_t T = (uint32_t)c->T;
    const int D = c->D;
    uint64_t M = 0;
    DevBuf b_seg, b_sum;
    if (int r = gather_level_segments(c, &M, b_seg, b_sum)) return r;
    *n_segments = M;
    if (n_recorded) *n_recorded = m.n_levels_recorded;
    if (!seg_len) return 0;
    std::vector<uint32_t> h_seg(M);
    std::vector<double> h_sum(M * 2 * D);
    HIPCHK(hipMemcpyAsync(h_seg.data(), b_seg.get(), M * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(h_sum.data(), b_sum.get(), M * 2 * D * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    lengths_of(h_seg.data(), M, T, seg_len);
    for (int d = 0; d < D; ++d) {
        if (sum) memcpy(sum + (uint64_t)d * M, h_sum.data() + (uint64_t)(2 * d) * M, M * sizeof(double));
        if (sum_sq) memcpy(sum_sq + (uint64_t)d * M, h_sum.data() + (uint64_t)(2 * d + 1) * M, M * sizeof(double));
    }
    return 0;
}

int hml_levels_dense_device(hml_ctx* c, void* out_dev) {
    NEED_MODEL();
    if (!out_dev) return set_err(HML_ERR_ARG, "null argument");
    hml_model m; if (int r = recorder_ready(c, HML_REC_LEVELS, &m)) return r;
    const uint32_t T = (uint32_t)c->T;
    const int D = c->D;
    uint64_t M = 0;
    DevBuf b_seg, b_sum, b_ms;
    if (int r = gather_level_segments(c, &M, b_seg, b_sum)) return r;
    HIPCHK(b_ms.alloc(M * 2 * D * sizeof(float)));
    hipLaunchKernelGGL(hml_k_levels_mean_sd, dim3(grid_for(M, 256, 1, 16384)), dim3(256), 0, c->stream, b_sum.as<double>(), (uint32_t)M, D,
                       m.n_levels_recorded, b_ms.as<float>());
    hipLaunchKernelGGL(hml_k_levels_expand, dim3(grid_for(T, 256, 1, 65536)), dim3(256), 0, c->stream, b_ms.as<float>(), b_seg.as<uint32_t>(),
                       (uint32_t)M, T, 2 * D, (float*)out_dev);
    KLAUNCH_CHECK();
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

int hml_levels_merge(hml_ctx* dst, hml_ctx* src) { return recorder_merge(dst, src, HML_REC_LEVELS); }

}  // extern "C"

// ---------------------------------------------------------------------------------------- agreement of chains (hml_k_agree.h)

// how the three agreement calls begin: the arguments hold n distinct contexts of one device over the same positions and
// dimensions that recorded the same N >= 2 levels; every context settled, the device bound.  The work runs on ctxs[0]'s stream.
static int agreement_ready(hml_ctx* const* ctxs, int n, uint64_t* N_out) {
    if (!ctxs) return set_err(HML_ERR_ARG, "null argument");
    if (n < 2 || n > HML_AGREE_MAX_CHAINS) return set_err(HML_ERR_ARG, "the agreement of the emission levels is taken over 2 to 64 chains");
    for (int i = 0; i < n; ++i) {
        if (!ctxs[i]) return set_err(HML_ERR_ARG, "null argument");
        if (!ctxs[i]->model_set) return set_err(HML_ERR_ARG, "model not set");
        for (int j = 0; j < i; ++j)
            if (ctxs[j] == ctxs[i]) return set_err(HML_ERR_ARG, "a context was given twice: the agreement of a chain with itself says nothing");
    }
    const hml_ctx* a = ctxs[0];
    for (int i = 1; i < n; ++i) {
        if (ctxs[i]->device != a->device)
            return set_err(HML_ERR_ARG, "the agreement of the emission levels of chains on different GPUs is not computed yet: run the chains of one rhat file on one GPU");
        if (ctxs[i]->T != a->T || ctxs[i]->D != a->D)
            return set_err(HML_ERR_ARG, "the agreement of the emission levels can only be computed between chains over the same positions and dimensions");
    }
    for (int i = 0; i < n; ++i)
        if (!ctxs[i]->rec[HML_REC_LEVELS].asked) return recorder_none(HML_REC_LEVELS, i == 0 ? "the first" : "a");
    if (int r = ctx_bind(ctxs[0])) return r;
    for (int i = 0; i < n; ++i) { if (int r = hml_settle(ctxs[i])) return r; }
    uint64_t N = 0;
    for (int i = 0; i < n; ++i) {
        hml_ctx* c = ctxs[i];
        if (int r = check_device_error(c)) return r;
        unsigned long long Ni = 0;   // (a context that was asked but has no buffers yet recorded nothing)
        if (c->rec[HML_REC_LEVELS].d_acc) {
            HIPCHK(hipMemcpyAsync(&Ni, recorder_counter(c, HML_REC_LEVELS), sizeof Ni, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));
        }
        if (Ni < 2) return set_err(HML_ERR_ARG, "the agreement of the emission levels needs at least two recorded sweeps in every chain");
        if (i > 0 && Ni != N) return set_err(HML_ERR_ARG, "the agreement of the emission levels needs the same number of recorded sweeps in every chain");
        N = Ni;
    }
    *N_out = N;
    return 0;
}

// the union of the chains' level boundaries on the device: starts d_useg[U], and the chains' bitmaps in `ch`
static int agreement_union(hml_ctx* const* ctxs, int n, hml_agree_chains& ch, uint64_t* U_out, DevBuf& d_useg) {
    hml_ctx* a = ctxs[0];
    const uint32_t T = (uint32_t)a->T;
    const uint32_t words = (uint32_t)((a->T + 32) / 32);   // (what ensure_recorder_buffers allocates)
    memset(&ch, 0, sizeof ch);
    for (int i = 0; i < n; ++i) ch.boundary[i] = ctxs[i]->rec[HML_REC_LEVELS].d_boundary;
    DevBuf d_or;
    HIPCHK(d_or.alloc((uint64_t)words * sizeof(uint32_t)));
    hipLaunchKernelGGL(hml_k_agree_or, dim3(grid_for(words, 256, 1, 16384)), dim3(256), 0, a->stream, ch, n, words, d_or.as<uint32_t>());
    KLAUNCH_CHECK();
    return compact_boundaries(a->stream, d_or.as<uint32_t>(), T, a->n_spans, U_out, d_useg);   // (synchronises: d_or may go)
}

// within, between and rhat per union segment and dimension, [D][U] each, and rhat as floats, on the device
struct hml_agreement {
    uint64_t U = 0, N = 0;
    DevBuf useg, within, between, rhat, rhat_f;
};
static int agreement_segments(hml_ctx* const* ctxs, int n, hml_agreement& ag) {
    hml_ctx* a = ctxs[0];
    const int D = a->D;
    hml_agree_chains ch;
    if (int r = agreement_union(ctxs, n, ch, &ag.U, ag.useg)) return r;
    const uint64_t U = ag.U;
    // each chain's own segments: the sums hml_levels_rle returns (on the chain's stream, idle again when the call returns)
    std::vector<DevBuf> b_seg(n), b_sum(n);
    for (int i = 0; i < n; ++i) {
        uint64_t M = 0;
        if (int r = gather_level_segments(ctxs[i], &M, b_seg[i], b_sum[i])) return r;
        b_seg[i].free();   // (the rank takes the place of the starts)
        ch.sum[i] = b_sum[i].as<double>();
        ch.M[i] = (uint32_t)M;
    }
    // the chains' segments under the union's, by rank: flags, then the fixed scan over each chain's row
    DevBuf b_flag, b_rank;
    HIPCHK(b_flag.alloc((uint64_t)n * U * sizeof(uint8_t)));
    HIPCHK(b_rank.alloc((uint64_t)n * U * sizeof(uint32_t)));
    const dim3 grid(grid_for(U, 256, 1, 16384));
    hipLaunchKernelGGL(hml_k_agree_flags, grid, dim3(256), 0, a->stream, ch, n, ag.useg.as<uint32_t>(), (uint32_t)U, b_flag.as<uint8_t>());
    KLAUNCH_CHECK();
    if (int r = scan_rows<uint8_t, uint32_t, false>(a->stream, b_flag.as<uint8_t>(), U, n, b_rank.as<uint32_t>())) return r;
    HIPCHK(ag.within.alloc((uint64_t)D * U * sizeof(double)));
    HIPCHK(ag.between.alloc((uint64_t)D * U * sizeof(double)));
    HIPCHK(ag.rhat.alloc((uint64_t)D * U * sizeof(double)));
    HIPCHK(ag.rhat_f.alloc((uint64_t)D * U * sizeof(float)));
    hipLaunchKernelGGL(hml_k_agree_eval, grid, dim3(256), 0, a->stream, ch, n, D, b_rank.as<uint32_t>(), (uint32_t)U, (unsigned long long)ag.N,
                       ag.within.as<double>(), ag.between.as<double>(), ag.rhat.as<double>(), ag.rhat_f.as<float>());
    KLAUNCH_CHECK();
    HIPCHK(hipStreamSynchronize(a->stream));   // (the chains' sums, the flags and the ranks go with this frame)
    return 0;
}

extern "C" {

int hml_levels_agreement_rle(hml_ctx* const* ctxs, int n, uint64_t* n_segments, uint64_t* n_recorded, uint64_t* seg_len, double* within,
                             double* between, double* rhat) {
    if (!n_segments) return set_err(HML_ERR_ARG, "null argument");
    hml_agreement ag;
    if (int r = agreement_ready(ctxs, n, &ag.N)) return r;
    if (n_recorded) *n_recorded = ag.N;
    if (!seg_len) {   // the sizes: the union alone
        hml_agree_chains ch;
        return agreement_union(ctxs, n, ch, n_segments, ag.useg);
    }
    if (int r = agreement_segments(ctxs, n, ag)) return r;
    hml_ctx* a = ctxs[0];
    const uint64_t U = ag.U, bytes = (uint64_t)a->D * U * sizeof(double);
    *n_segments = U;
    std::vector<uint32_t> h_seg(U);
    HIPCHK(hipMemcpyAsync(h_seg.data(), ag.useg.get(), U * sizeof(uint32_t), hipMemcpyDeviceToHost, a->stream));
    if (within) HIPCHK(hipMemcpyAsync(within, ag.within.get(), bytes, hipMemcpyDeviceToHost, a->stream));
    if (between) HIPCHK(hipMemcpyAsync(between, ag.between.get(), bytes, hipMemcpyDeviceToHost, a->stream));
    if (rhat) HIPCHK(hipMemcpyAsync(rhat, ag.rhat.get(), bytes, hipMemcpyDeviceToHost, a->stream));
    HIPCHK(hipStreamSynchronize(a->stream));
    lengths_of(h_seg.data(), U, (uint32_t)a->T, seg_len);
    return 0;
}

int hml_levels_agreement_dense_device(hml_ctx* const* ctxs, int n, void* out_dev) {
    if (!out_dev) return set_err(HML_ERR_ARG, "null argument");
    hml_agreement ag;
    if (int r = agreement_ready(ctxs, n, &ag.N)) return r;
    if (int r = agreement_segments(ctxs, n, ag)) return r;
    hml_ctx* a = ctxs[0];
    const uint32_t T = (uint32_t)a->T;
    hipLaunchKernelGGL(hml_k_levels_expand, dim3(grid_for(T, 256, 1, 65536)), dim3(256), 0, a->stream, ag.rhat_f.as<float>(), ag.useg.as<uint32_t>(),
                       (uint32_t)ag.U, T, a->D, (float*)out_dev);
    KLAUNCH_CHECK();
    HIPCHK(hipStreamSynchronize(a->stream));
    return 0;
}

int hml_levels_agreement_summary(hml_ctx* const* ctxs, int n, double threshold, uint64_t* n_above, double* max_finite, uint64_t* n_infinite) {
    if (!n_above || !max_finite || !n_infinite) return set_err(HML_ERR_ARG, "null argument");
    hml_agreement ag;
    if (int r = agreement_ready(ctxs, n, &ag.N)) return r;
    if (int r = agreement_segments(ctxs, n, ag)) return r;
    hml_ctx* a = ctxs[0];
    const int D = a->D;
    const int blocks = grid_for(ag.U, 1024, 1, 256);
    DevBuf b_cnt, b_max;
    HIPCHK(b_cnt.alloc((uint64_t)blocks * D * 2 * sizeof(unsigned long long)));
    HIPCHK(b_max.alloc((uint64_t)blocks * D * sizeof(double)));
    hipLaunchKernelGGL(hml_k_agree_summary, dim3(blocks), dim3(256), 0, a->stream, ag.rhat.as<double>(), ag.useg.as<uint32_t>(), (uint32_t)ag.U, (uint32_t)a->T,
                       D, threshold, b_cnt.as<unsigned long long>(), b_max.as<double>());
    KLAUNCH_CHECK();
    std::vector<unsigned long long> h_cnt((size_t)blocks * D * 2);
    std::vector<double> h_max((size_t)blocks * D);
    HIPCHK(hipMemcpyAsync(h_cnt.data(), b_cnt.get(), h_cnt.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, a->stream));
    HIPCHK(hipMemcpyAsync(h_max.data(), b_max.get(), h_max.size() * sizeof(double), hipMemcpyDeviceToHost, a->stream));
    HIPCHK(hipStreamSynchronize(a->stream));
    // the second stage: integers and a maximum - the same answer in any order
    for (int d = 0; d < D; ++d) {
        n_above[d] = 0; n_infinite[d] = 0; max_finite[d] = 0.0;
        for (int b = 0; b < blocks; ++b) {
            n_above[d] += h_cnt[((size_t)b * D + d) * 2];
            n_infinite[d] += h_cnt[((size_t)b * D + d) * 2 + 1];
            max_finite[d] = std::max(max_finite[d], h_max[(size_t)b * D + d]);
        }
    }
    return 0;
}

// ---------------------------------------------------------------------------------------- breakpoints (hml_k_breaks.h)
}  // extern "C"

// exclusive 64-bit prefix sums of M 32-bit values on `s`: d_pre[M + 1] (allocated here), d_pre[M] = the total
static int breaks_scan(hipStream_t s, const uint32_t* d_v, uint64_t M, DevBuf& d_pre) {
    HIPCHK(d_pre.alloc((M + 1) * sizeof(unsigned long long)));
    return scan_rows<uint32_t, unsigned long long, true>(s, d_v, M, 1, d_pre.as<unsigned long long>());
}

// the positions with a count, ascending, on the device: d_list[1 + M] - entry 0 is the position 0 that the compaction kernels
// always emit (never a breakpoint), the M break positions follow
static int compact_break_positions(hml_ctx* c, uint64_t* M_out, DevBuf& d_list) {
    uint64_t n = 0;
    if (int r = compact_boundaries(c->stream, c->rec[HML_REC_BREAKS].d_boundary, (uint32_t)c->T, c->n_spans, &n, d_list)) return r;
    *M_out = n - 1;   // (position 0 always counts)
    return 0;
}

// C[pos] for the M break positions of d_list into d_cnt[M] (allocated here with one spare entry)
static int gather_break_counts(hml_ctx* c, const DevBuf& d_list, uint64_t M, DevBuf& d_cnt) {
    HIPCHK(d_cnt.alloc((M + 1) * sizeof(uint32_t)));
    if (M) hipLaunchKernelGGL(hml_k_rec_gather<uint32_t>, dim3(grid_for(M, 256, 1, 16384)), dim3(256), 0, c->stream, c->rec[HML_REC_BREAKS].acc<uint32_t>(), (uint32_t)c->T, 1,
                              d_list.as<uint32_t>() + 1, (uint32_t)M, d_cnt.as<uint32_t>());
    KLAUNCH_CHECK();
    return 0;
}

// break positions d_list[1 + M] (see above), their counts d_cnt[M] and the exclusive sums of the counts d_pre[M + 1]
static int gather_breaks(hml_ctx* c, uint64_t* M_out, DevBuf& d_list, DevBuf& d_cnt, DevBuf& d_pre) {
    uint64_t M = 0;
    if (int r = compact_break_positions(c, &M, d_list)) return r;
    if (int r = gather_break_counts(c, d_list, M, d_cnt)) return r;
    if (int r = breaks_scan(c->stream, d_cnt.as<uint32_t>(), M, d_pre)) return r;
    *M_out = M;
    return 0;
}

extern "C" {

int hml_breaks_list(hml_ctx* c, uint64_t* n_breaks, uint64_t* n_recorded, uint32_t* pos, uint32_t* count) {
    NEED_MODEL();
    if (!n_breaks) return set_err(HML_ERR_ARG, "null argument");
    hml_model m; if (int r = recorder_ready(c, HML_REC_BREAKS, &m)) return r;
    uint64_t M = 0;
    DevBuf b_list, b_cnt;
    if (int r = compact_break_positions(c, &M, b_list)) return r;
    *n_breaks = M;
    if (n_recorded) *n_recorded = m.n_breaks_recorded;
    if (!pos || M == 0) return 0;
    HIPCHK(hipMemcpyAsync(pos, b_list.as<uint32_t>() + 1, M * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    if (count) {
        if (int r = gather_break_counts(c, b_list, M, b_cnt)) return r;
        HIPCHK(hipMemcpyAsync(count, b_cnt.get(), M * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

int hml_breaks_dense_device(hml_ctx* c, void* out_dev, uint32_t window) {
    NEED_MODEL();
    if (!out_dev) return set_err(HML_ERR_ARG, "null argument");
    hml_model m; if (int r = recorder_ready(c, HML_REC_BREAKS, &m)) return r;
    uint64_t M = 0;
    DevBuf b_list, b_cnt, b_pre;
    if (int r = gather_breaks(c, &M, b_list, b_cnt, b_pre)) return r;
    const uint32_t T = (uint32_t)c->T;
    hipLaunchKernelGGL(hml_k_breaks_dense, dim3(grid_for(T, 256, 1, 65536)), dim3(256), 0, c->stream, b_list.as<uint32_t>() + 1, b_pre.as<unsigned long long>(),
                       (uint32_t)M, T, window, m.n_breaks_recorded, (float*)out_dev);
    KLAUNCH_CHECK();
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

int hml_breaks_consensus(hml_ctx* c, uint32_t window, uint64_t min_count, uint64_t* n_selected, uint32_t* pos, uint64_t* mass, uint32_t* peak) {
    NEED_MODEL();
    if (!n_selected) return set_err(HML_ERR_ARG, "null argument");
    hml_model m; if (int r = recorder_ready(c, HML_REC_BREAKS, &m)) return r;
    uint64_t M = 0;
    DevBuf b_list, b_cnt, b_pre, b_mass, b_sel, b_where, b_opos, b_omass, b_opeak;
    if (int r = gather_breaks(c, &M, b_list, b_cnt, b_pre)) return r;
    *n_selected = 0;
    if (M == 0) return 0;
    HIPCHK(b_mass.alloc(M * sizeof(unsigned long long)));
    HIPCHK(b_sel.alloc(M * sizeof(uint32_t)));
    const uint32_t* d_pos = b_list.as<uint32_t>() + 1;
    hipLaunchKernelGGL(hml_k_breaks_select, dim3(grid_for(M, 256, 1, 16384)), dim3(256), 0, c->stream, d_pos, b_cnt.as<uint32_t>(), b_pre.as<unsigned long long>(),
                       (uint32_t)M, window, (unsigned long long)(min_count > 1 ? min_count : 1), b_mass.as<unsigned long long>(), b_sel.as<uint32_t>());
    KLAUNCH_CHECK();
    if (int r = breaks_scan(c->stream, b_sel.as<uint32_t>(), M, b_where)) return r;
    unsigned long long S = 0;
    HIPCHK(hipMemcpyAsync(&S, b_where.as<unsigned long long>() + M, sizeof S, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    *n_selected = S;
    if (!pos || S == 0) return 0;
    HIPCHK(b_opos.alloc(S * sizeof(uint32_t)));
    HIPCHK(b_omass.alloc(S * sizeof(unsigned long long)));
    HIPCHK(b_opeak.alloc(S * sizeof(uint32_t)));
    hipLaunchKernelGGL(hml_k_breaks_compact, dim3(grid_for(M, 256, 1, 16384)), dim3(256), 0, c->stream, d_pos, b_cnt.as<uint32_t>(), b_mass.as<unsigned long long>(),
                       b_sel.as<uint32_t>(), b_where.as<unsigned long long>(), (uint32_t)M, b_opos.as<uint32_t>(), b_omass.as<unsigned long long>(), b_opeak.as<uint32_t>());
    KLAUNCH_CHECK();
    HIPCHK(hipMemcpyAsync(pos, b_opos.get(), S * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    if (mass) HIPCHK(hipMemcpyAsync(mass, b_omass.get(), S * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    if (peak) HIPCHK(hipMemcpyAsync(peak, b_opeak.get(), S * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

int hml_breaks_merge(hml_ctx* dst, hml_ctx* src) { return recorder_merge(dst, src, HML_REC_BREAKS); }

int hml_levels_on_segments(hml_ctx* c, uint64_t n_cuts, const uint32_t* cuts, double* sum, double* sum_sq) {
    NEED_MODEL();
    if (n_cuts && !cuts) return set_err(HML_ERR_ARG, "null argument");
    const uint32_t T = (uint32_t)c->T;
    if (n_cuts >= T) return set_err(HML_ERR_ARG, "more cuts than positions");
    for (uint64_t i = 0; i < n_cuts; ++i) {
        if (cuts[i] == 0 || cuts[i] >= T) return set_err(HML_ERR_ARG, "a cut must lie inside (0, T)");
        if (i > 0 && cuts[i] <= cuts[i - 1]) return set_err(HML_ERR_ARG, "the cuts must be strictly ascending");
    }
    hml_model m; if (int r = recorder_ready(c, HML_REC_LEVELS, &m)) return r;
    const int D = c->D, rows = 2 * D;
    uint64_t M = 0;
    DevBuf b_seg, b_val, b_w, b_cuts, b_out;
    if (int r = gather_level_segments(c, &M, b_seg, b_val)) return r;
    const uint64_t n_seg = n_cuts + 1;
    HIPCHK(b_w.alloc(M * rows * sizeof(double)));
    HIPCHK(b_cuts.alloc((n_cuts + 1) * sizeof(uint32_t)));
    HIPCHK(b_out.alloc(n_seg * rows * sizeof(double)));
    if (n_cuts) HIPCHK(hipMemcpyAsync(b_cuts.get(), cuts, n_cuts * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(hml_k_levels_weigh, dim3(grid_for(M, 256, 1, 16384)), dim3(256), 0, c->stream, b_val.as<double>(), b_seg.as<uint32_t>(), (uint32_t)M, T, rows, b_w.as<double>());
    // the fixed-shape scan of the levels' read-out, now over len_i * value_i
    if (int r = scan_rows<double, double, false>(c->stream, b_w.as<double>(), M, rows, b_w.as<double>())) return r;
    hipLaunchKernelGGL(hml_k_levels_on_segments, dim3(grid_for(n_seg, 256, 1, 16384)), dim3(256), 0, c->stream, b_val.as<double>(), b_w.as<double>(), b_seg.as<uint32_t>(),
                       (uint32_t)M, T, rows, b_cuts.as<uint32_t>(), (uint32_t)n_cuts, b_out.as<double>());
    KLAUNCH_CHECK();
    std::vector<double> h_out(n_seg * rows);
    HIPCHK(hipMemcpyAsync(h_out.data(), b_out.get(), n_seg * rows * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (int d = 0; d < D; ++d) {
        if (sum) memcpy(sum + (uint64_t)d * n_seg, h_out.data() + (uint64_t)(2 * d) * n_seg, n_seg * sizeof(double));
        if (sum_sq) memcpy(sum_sq + (uint64_t)d * n_seg, h_out.data() + (uint64_t)(2 * d + 1) * n_seg, n_seg * sizeof(double));
    }
    return 0;
}

// ---------------------------------------------------------------------------------------- level bands (hml_k_bands.h)
int hml_bands_rle(hml_ctx* c, uint64_t* n_segments, int* n_columns, uint64_t* n_recorded, uint64_t* seg_len, int32_t* counts) {
    NEED_MODEL();
    if (!n_segments) return set_err(HML_ERR_ARG, "null argument");
    hml_model m; if (int r = recorder_ready(c, HML_REC_BANDS, &m)) return r;
    const hml_count_table tab = band_table(c);
    uint64_t M = 0;
    DevBuf b_seg, b_g;
    if (int r = table_segments(c, tab, &M, b_seg, b_g)) return r;
    *n_segments = M;
    if (n_columns) *n_columns = tab.ncol;
    if (n_recorded) *n_recorded = m.n_bands_recorded;
    if (!seg_len) return 0;
    return table_rle(c, tab, M, b_seg, b_g, tab.ncol, seg_len, counts);
}

int hml_bands_dense_device(hml_ctx* c, void* out_dev, int cumulative) {
    NEED_MODEL();
    if (!out_dev) return set_err(HML_ERR_ARG, "null argument");
    hml_model m; if (int r = recorder_ready(c, HML_REC_BANDS, &m)) return r;
    const uint32_t T = (uint32_t)c->T;
    int32_t* out = (int32_t*)out_dev;
    DevBuf b_cs;
    if (int r = table_dense(c, band_table(c), nullptr, out, b_cs)) return r;
    if (cumulative) hipLaunchKernelGGL(hml_k_bands_cumulate, dim3(grid_for(T, 256, 1, 65536)), dim3(256), 0, c->stream, out, T, c->D, c->n_band_edges + 1);
    KLAUNCH_CHECK();
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

int hml_bands_call(hml_ctx* c, uint64_t rank, uint64_t* n_runs, uint64_t* run_len, int32_t* run_band) {
    NEED_MODEL();
    if (!n_runs) return set_err(HML_ERR_ARG, "null argument");
    hml_model m; if (int r = recorder_ready(c, HML_REC_BANDS, &m)) return r;
    if (rank > m.n_bands_recorded) return set_err(HML_ERR_ARG, "hml_bands_call: the rank must be 0 (the most probable band) or between 1 and the number of recorded sweeps");
    const int D = c->D, nb = c->n_band_edges + 1;
    std::vector<int16_t> keys;
    auto pick = [&](const int32_t* d_g, uint32_t M, const int32_t* d_cs, uint32_t n_chunks, int16_t* d_key) {
        hipLaunchKernelGGL(hml_k_bands_pick, dim3(n_chunks), dim3(256), 0, c->stream, d_g, M, D, nb, d_cs, n_chunks, (unsigned long long)rank, d_key);
    };
    if (int r = table_runs(c, band_table(c), pick, n_runs, run_len, keys)) return r;
    if (!run_len || !run_band) return 0;
    const uint64_t R = keys.size();
    for (uint64_t r = 0; r < R; ++r) {
        uint32_t key = (uint16_t)keys[r];   // (hml_k_bands_pick: the D calls as digits to the base of the bands per dimension)
        for (int d = 0; d < D; ++d) { run_band[(uint64_t)d * R + r] = (int32_t)(key % (uint32_t)nb); key /= (uint32_t)nb; }
    }
    return 0;
}

int hml_bands_merge(hml_ctx* dst, hml_ctx* src) { return recorder_merge(dst, src, HML_REC_BANDS); }

}  // extern "C"

// ---------------------------------------------------------------------------------------- regions (hml_k_regions.h)
// The accumulators are a few words per region: the read-out copies them, and sums from elsewhere - another chain, another
// GPU, another process - are added on the host, one addition per number, and written back.

// the regions, their accumulators and the chunk scratch on first use.  Ready before this returns: chains batched by
// hml_iterate_many run on their group's stream, not on their own.
int hml_regions_ensure(hml_ctx* c) {
    hml_regions& g = c->rg;
    if (g.d_acc) return 0;
    if (g.start.empty()) return set_err(HML_ERR_ARG, "regions: none were given");
    if (!g.checked) { if (int r = regions_fault(c)) return r; g.checked = true; }
    const uint64_t n = g.start.size();
    const uint64_t acc_bytes = regions_acc_words(c) * n * 8u;
    const uint64_t chunk_bytes = (uint64_t)regions_chunk_stride(c) * ((uint64_t)c->D * sizeof(double) + (1u + (uint64_t)c->D) * sizeof(uint32_t));
    HIPCHK(g.d_start.alloc(n));
    HIPCHK(g.d_end.alloc(n));
    HIPCHK(g.d_chunks.alloc(chunk_bytes));
    HIPCHK(g.d_acc.alloc(acc_bytes));
    HIPCHK(hipMemcpyAsync(g.d_start, g.start.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(g.d_end, g.end.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemsetAsync(g.d_chunks.get(), 0, chunk_bytes, c->stream));
    HIPCHK(hipMemsetAsync(g.d_acc.get(), 0, acc_bytes, c->stream));
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(c->stream, &cap) == hipSuccess && cap == hipStreamCaptureStatusNone) HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

// the three launches of a recorded sweep's regions, on stream `s`, behind the sweep's parameter update like the recorders
// above: chunk totals, their exclusive sums, a wavefront per region (the buffers exist: ensure_region_buffers)
void hml_regions_launch(hml_ctx* c, hipStream_t s, uint32_t hint, bool bracket) {
    const hml_band_edges ed = region_edges_of(c);
    const hml_regions_chunks ch = regions_chunk_views(c);
    const uint32_t n = (uint32_t)c->rg.start.size();
    // (bracket: `s` is the context's own stream - launch_recorders - and the three kernels get profile families of their own
    // inside the family "regions"; the batches of hml_iterate_many run on their group's stream and are never profiled)
    const int level = bracket ? 2 : 1 << 30;
    {
        ProfScope ps(c, "regions_chunks", level);
        hipLaunchKernelGGL(hml_k_regions_chunks, dim3(grid_for(hint, HML_RG_CHUNK, 1, 16384)), dim3(HML_RG_CHUNK), 0, s, c->d_q, c->d_starts, c->d_mdl, ed, ch);
    }
    {
        ProfScope ps(c, "regions_scan", level);
        hipLaunchKernelGGL(hml_k_regions_scan, dim3(1 + (ed.n > 0 ? 2 : 1) * c->D), dim3(1024), 0, s, c->d_mdl, ch);
    }
    {
        ProfScope ps(c, "regions_accumulate", level);
        hipLaunchKernelGGL(hml_k_regions_accumulate, dim3(grid_for(n, 4, 1, 16384)), dim3(256), 0, s, c->d_q, c->d_starts, c->d_mdl, ed, ch, c->rg.d_start, c->rg.d_end, n,
                           regions_acc_views(c));
    }
}


struct hml_regions_host {
    uint64_t n = 0, N = 0;
    int D = 1, ncol = 0;
    std::vector<unsigned long long> words;   // the device layout (hml_regions_acc)
    unsigned long long* whole() { return words.data(); }
    unsigned long long* breaks_sum() { return words.data() + n; }
    unsigned long long* breaks_sq() { return words.data() + 2 * n; }
    double* level_sum() { return reinterpret_cast<double*>(words.data() + 3 * n); }
    double* level_sq() { return level_sum() + (uint64_t)D * n; }
    unsigned long long* inband() { return words.data() + (3u + 2u * (uint64_t)D) * n; }
};

static int regions_fetch(hml_ctx* c, const char* whose, hml_regions_host& h) {
    if (!c || !c->model_set) return set_err(HML_ERR_ARG, "model not set");
    if (!c->rg.asked) return regions_none(whose);
    if (int r = ctx_bind(c)) return r;
    if (int r = hml_settle(c)) return r;
    if (int r = ensure_region_buffers(c)) return r;
    hml_model m;
    if (int r = fetch_model(c, &m)) return r;
    if (int r = model_fault(m)) return r;
    h.n = c->rg.start.size(); h.N = m.n_regions_recorded; h.D = c->D; h.ncol = regions_columns(c);
    h.words.resize(regions_acc_words(c) * h.n);
    HIPCHK(hipMemcpy(h.words.data(), c->rg.d_acc.get(), h.words.size() * 8u, hipMemcpyDeviceToHost));
    return 0;
}

// raw sums into the context's accumulators: integers add (breaks_sq saturates and stays there), a double gets one addition
static int regions_add_host(hml_ctx* c, uint64_t N, const uint64_t* whole, const uint64_t* breaks_sum, const uint64_t* breaks_sq, const double* level_sum,
                            const double* level_sq, const uint64_t* inband) {
    hml_regions_host h;
    if (int r = regions_fetch(c, "this", h)) return r;
    if (!whole || !breaks_sum || !breaks_sq || !level_sum || !level_sq || (h.ncol > 0 && !inband)) return set_err(HML_ERR_ARG, "null argument");
    for (uint64_t r = 0; r < h.n; ++r) {
        h.whole()[r] += whole[r];
        h.breaks_sum()[r] += breaks_sum[r];
        h.breaks_sq()[r] = hml_sat_add_u64(h.breaks_sq()[r], breaks_sq[r]);
    }
    for (uint64_t i = 0; i < (uint64_t)h.D * h.n; ++i) { h.level_sum()[i] += level_sum[i]; h.level_sq()[i] += level_sq[i]; }
    for (uint64_t i = 0; i < h.n * (uint64_t)h.ncol; ++i) h.inband()[i] += inband[i];
    const unsigned long long total = h.N + N;
    HIPCHK(hipMemcpy(c->rg.d_acc.get(), h.words.data(), h.words.size() * 8u, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(&c->d_mdl->n_regions_recorded, &total, sizeof total, hipMemcpyHostToDevice));
    return 0;
}

extern "C" {

int hml_regions_read(hml_ctx* c, uint64_t* n, int* n_columns, uint64_t* n_recorded, uint64_t* whole, uint64_t* breaks_sum, uint64_t* breaks_sq, double* level_sum,
                     double* level_sq, uint64_t* inband) {
    if (!n) return set_err(HML_ERR_ARG, "null argument");
    hml_regions_host h;
    if (int r = regions_fetch(c, "this", h)) return r;
    *n = h.n;
    if (n_columns) *n_columns = h.ncol;
    if (n_recorded) *n_recorded = h.N;
    if (whole) memcpy(whole, h.whole(), h.n * 8u);
    if (breaks_sum) memcpy(breaks_sum, h.breaks_sum(), h.n * 8u);
    if (breaks_sq) memcpy(breaks_sq, h.breaks_sq(), h.n * 8u);
    if (level_sum) memcpy(level_sum, h.level_sum(), (uint64_t)h.D * h.n * 8u);
    if (level_sq) memcpy(level_sq, h.level_sq(), (uint64_t)h.D * h.n * 8u);
    if (inband && h.ncol > 0) memcpy(inband, h.inband(), h.n * (uint64_t)h.ncol * 8u);
    return 0;
}

int hml_regions_add(hml_ctx* c, uint64_t n_recorded, const uint64_t* whole, const uint64_t* breaks_sum, const uint64_t* breaks_sq, const double* level_sum,
                    const double* level_sq, const uint64_t* inband) {
    return regions_add_host(c, n_recorded, whole, breaks_sum, breaks_sq, level_sum, level_sq, inband);
}

int hml_regions_merge(hml_ctx* dst, hml_ctx* src) {
    if (!dst || !src || !dst->model_set || !src->model_set) return set_err(HML_ERR_ARG, "model not set");
    if (dst == src) return set_err(HML_ERR_ARG, "a context cannot be merged into itself");
    if (dst->T != src->T || dst->D != src->D) return set_err(HML_ERR_ARG, "regions can only be merged between chains over the same positions and dimensions");
    if (!src->rg.asked) return regions_none("the source");
    if (!dst->rg.asked) return regions_none("the destination");
    if (!same_regions(dst, src->rg.start.size(), src->rg.start.data(), src->rg.end.data(), src->rg.n_edges, src->rg.edges))
        return set_err(HML_ERR_ARG, "regions can only be merged between chains with the same regions and edges, bit for bit");
    hml_regions_host h;
    if (int r = regions_fetch(src, "the source", h)) return r;   // (the two contexts may lie on different GPUs: the sums travel through the host)
    return regions_add_host(dst, h.N, (const uint64_t*)h.whole(), (const uint64_t*)h.breaks_sum(), (const uint64_t*)h.breaks_sq(), h.level_sum(), h.level_sq(),
                            (const uint64_t*)h.inband());
}

}  // extern "C"


// ---------------------------------------------------------------------------------------- sparse payloads (hml_k_rec_payload.h)
static_assert(HML_RECORDING_LEVELS == HML_REC_LEVELS && HML_RECORDING_BREAKS == HML_REC_BREAKS && HML_RECORDING_BANDS == HML_REC_BANDS,
              "the public kinds carry the values of the internal ones");

static uint64_t payload_bytes(uint64_t M, uint64_t rows, uint64_t cell) { return HML_RECPAY_FIXED_BYTES + 8u * ((M + 1u) / 2u) + rows * M * cell; }
static int payload_kind(int kind) {
    return kind >= 0 && kind < HML_REC_KINDS ? 0 : set_err(HML_ERR_ARG, "the kind of a recording is HML_RECORDING_LEVELS, HML_RECORDING_BREAKS or HML_RECORDING_BANDS");
}

// What an export of the context's recording holds: the chain settled, its M positions on the device (d_seg owns them, *d_pos
// points at the first) - compact_boundaries' list, for breaks without the position 0 it always emits; no position at all
// from a recorder that has recorded no sweep.
static int payload_positions(hml_ctx* c, int kind, uint64_t* M_out, DevBuf& d_seg, const uint32_t** d_pos) {
    if (!c->rec[kind].asked) return recorder_none(kind, "this");
    if (int r = hml_settle(c)) return r;
    if (int r = check_device_error(c)) return r;
    if (int r = ensure_recorder_buffers(c, kind)) return r;
    unsigned long long N = 0;
    HIPCHK(hipMemcpyAsync(&N, recorder_counter(c, kind), sizeof N, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    *M_out = 0; *d_pos = nullptr;
    if (N == 0) return 0;
    uint64_t M = 0;
    if (int r = compact_boundaries(c->stream, c->rec[kind].d_boundary, (uint32_t)c->T, c->n_spans, &M, d_seg)) return r;
    *d_pos = d_seg.as<uint32_t>();
    if (kind == HML_REC_BREAKS) { ++*d_pos; --M; }
    *M_out = M;
    return 0;
}

// ... and the export itself; *n_bytes is set also when the capacity is too small (nothing is written then)
static int payload_export(hml_ctx* c, int kind, void* payload_dev, uint64_t capacity, uint64_t* n_bytes) {
    uint64_t M = 0;
    DevBuf b_seg;
    const uint32_t* d_pos = nullptr;
    if (int r = payload_positions(c, kind, &M, b_seg, &d_pos)) return r;
    const uint64_t rows = (uint64_t)recorder_rows(c, kind), cell = hml_recorder_kinds[kind].elem;
    const uint64_t bytes = payload_bytes(M, rows, cell);
    if (n_bytes) *n_bytes = bytes;
    if (!payload_dev) return set_err(HML_ERR_ARG, "null argument");
    if (capacity < bytes) return set_err(HML_ERR_ARG, "hml_recording_export: the buffer is smaller than hml_recording_payload_size says");
    if ((uintptr_t)payload_dev % 8u) return set_err(HML_ERR_ARG, "a recording's payload must be aligned to 8 bytes");
    const uint32_t T = (uint32_t)c->T;
    hml_band_edges ed;
    memset(&ed, 0, sizeof ed);
    if (kind == HML_REC_BANDS) ed = band_edges_of(c);
    char* const out = (char*)payload_dev;
    hipLaunchKernelGGL(hml_k_recpay_header, dim3(1), dim3(64), 0, c->stream, (unsigned long long*)out, (unsigned long long)kind, (unsigned long long)T,
                       (unsigned long long)rows, (unsigned long long)M, (const unsigned long long*)recorder_counter(c, kind), (unsigned long long)cell, ed);
    KLAUNCH_CHECK();
    if (M) {
        HIPCHK(hipMemcpyAsync(out + HML_RECPAY_FIXED_BYTES, d_pos, M * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream));
        char* const cells = out + HML_RECPAY_FIXED_BYTES + 8u * ((M + 1u) / 2u);
        const dim3 grid(grid_for(M, 256, 1, 16384));
        const hml_recorder& rec = c->rec[kind];
        if (kind == HML_REC_LEVELS)
            hipLaunchKernelGGL(hml_k_rec_gather<double>, grid, dim3(256), 0, c->stream, rec.acc<double>(), T, (int)rows, d_pos, (uint32_t)M, (double*)cells);
        else if (kind == HML_REC_BREAKS)
            hipLaunchKernelGGL(hml_k_rec_gather<uint32_t>, grid, dim3(256), 0, c->stream, rec.acc<uint32_t>(), T, (int)rows, d_pos, (uint32_t)M, (uint32_t*)cells);
        else
            hipLaunchKernelGGL(hml_k_rec_gather<int32_t>, grid, dim3(256), 0, c->stream, rec.acc<int32_t>(), T, (int)rows, d_pos, (uint32_t)M, (int32_t*)cells);
        KLAUNCH_CHECK();
    }
    HIPCHK(hipStreamSynchronize(c->stream));   // (the positions go with this frame)
    return 0;
}

// hml_recording_merge_payload.  Everything is checked before anything is written: the header on the host, the positions by
// hml_k_recpay_check on the device.
static int payload_merge(hml_ctx* dst, int kind, const void* payload_dev, uint64_t n_bytes) {
    if (!dst || !dst->model_set) return set_err(HML_ERR_ARG, "model not set");
    if (int r = payload_kind(kind)) return r;
    if (!payload_dev) return set_err(HML_ERR_ARG, "null argument");
    if ((uintptr_t)payload_dev % 8u) return set_err(HML_ERR_ARG, "a recording's payload must be aligned to 8 bytes");
    if (n_bytes < HML_RECPAY_FIXED_BYTES) return set_err(HML_ERR_ARG, "the payload is shorter than its header");
    if (int r = ctx_bind(dst)) return r;
    if (int r = hml_settle(dst)) return r;
    struct { uint64_t h[HML_RECPAY_HEADER_WORDS]; float edges[HML_RECPAY_EDGE_SLOTS]; } head;
    static_assert(sizeof head == HML_RECPAY_FIXED_BYTES, "header and edges are 192 bytes");
    HIPCHK(hipMemcpyAsync(&head, payload_dev, sizeof head, hipMemcpyDeviceToHost, dst->stream));
    HIPCHK(hipStreamSynchronize(dst->stream));
    const hml_recorder_kind& rk = hml_recorder_kinds[kind];
    const uint64_t T = head.h[2], rows = head.h[3], M = head.h[4], N = head.h[5], n_edges = head.h[7];
    if (head.h[0] != HML_RECPAY_MAGIC) return set_err(HML_ERR_ARG, "the payload does not begin with the magic number of a recording (HMLREC1)");
    if (head.h[1] != (uint64_t)kind) return set_err(HML_ERR_ARG, std::string("the payload holds another kind of recording, not ") + rk.noun);
    if (T != dst->T) return set_err(HML_ERR_ARG, std::string("the payload's ") + rk.noun + " were recorded over another number of positions than the destination's");
    if (kind == HML_REC_BANDS && (n_edges < 1 || n_edges > HML_MAX_BAND_EDGES)) return set_err(HML_ERR_ARG, "the payload's number of band edges must be between 1 and 31");
    if (kind != HML_REC_BANDS && n_edges != 0) return set_err(HML_ERR_ARG, "the payload carries band edges but is not a bands payload");
    const uint64_t want_rows = kind == HML_REC_LEVELS ? 2u * (uint64_t)dst->D : kind == HML_REC_BREAKS ? 1u : (uint64_t)dst->D * (n_edges + 1u);
    if (rows != want_rows || rows > (kind == HML_REC_LEVELS ? 2u * HML_MAX_D : (uint64_t)HML_CAP_K))
        return set_err(HML_ERR_ARG, std::string("the payload's rows do not match the destination's dimensions") + (kind == HML_REC_BANDS ? " and the payload's edges" : ""));
    if (head.h[6] != rk.elem) return set_err(HML_ERR_ARG, std::string("the payload's cell size is not the one of ") + rk.noun);
    if (M > T) return set_err(HML_ERR_ARG, "the payload lists more positions than there are");
    if (n_bytes != payload_bytes(M, rows, rk.elem)) return set_err(HML_ERR_ARG, "the payload's size in bytes is not the one its header implies");
    bool take_edges = false;
    if (kind == HML_REC_BANDS) {
        for (uint64_t j = 0; j < HML_RECPAY_EDGE_SLOTS; ++j) {
            uint32_t bits; memcpy(&bits, &head.edges[j], 4);
            if (j >= n_edges ? bits != 0u : !std::isfinite(head.edges[j]) || (j > 0 && !(head.edges[j - 1] < head.edges[j])))
                return set_err(HML_ERR_ARG, "the payload's band edges must be finite and strictly ascending, followed by zeros");
        }
        if (!same_band_edges(dst, (int)n_edges, head.edges)) {
            // a destination that was never asked takes the payload's edges; any other difference is refused
            if (dst->rec[kind].asked || dst->rec[kind].d_acc) return set_err(HML_ERR_ARG, "level bands can only be merged between chains with the same edges, bit for bit");
            take_edges = true;
        }
    }
    const char* const base = (const char*)payload_dev;
    const uint32_t* const d_pos = (const uint32_t*)(base + HML_RECPAY_FIXED_BYTES);
    const char* const cells = base + HML_RECPAY_FIXED_BYTES + 8u * ((M + 1u) / 2u);
    if (M) {
        DevBuf b_flag;
        HIPCHK(b_flag.alloc(sizeof(uint32_t)));
        HIPCHK(hipMemsetAsync(b_flag.get(), 0, sizeof(uint32_t), dst->stream));
        hipLaunchKernelGGL(hml_k_recpay_check, dim3(grid_for(M, 256, 1, 1024)), dim3(256), 0, dst->stream, d_pos, (uint32_t)M, (uint32_t)T, kind == HML_REC_BREAKS ? 1u : 0u,
                           b_flag.as<uint32_t>());
        KLAUNCH_CHECK();
        uint32_t bad = 0;
        HIPCHK(hipMemcpyAsync(&bad, b_flag.get(), sizeof bad, hipMemcpyDeviceToHost, dst->stream));
        HIPCHK(hipStreamSynchronize(dst->stream));
        if (bad & HML_RECPAY_BAD_RANGE) return set_err(HML_ERR_ARG, "the payload lists a position beyond the last one");
        if (bad & HML_RECPAY_BAD_ZERO) return set_err(HML_ERR_ARG, "a breaks payload lists position 0, which is never a breakpoint");
        if (bad & HML_RECPAY_BAD_ORDER) return set_err(HML_ERR_ARG, "the payload's positions are not strictly ascending");
    }
    // valid: from here on the destination changes
    if (take_edges) {
        dst->n_band_edges = (int)n_edges;
        memset(dst->band_edges, 0, sizeof dst->band_edges);
        memcpy(dst->band_edges, head.edges, (size_t)n_edges * sizeof(float));
    }
    if (int r = ensure_recorder_buffers(dst, kind)) return r;
    dst->rec[kind].asked = true;
    const hml_recorder& rd = dst->rec[kind];
    const dim3 grid(grid_for(M, 256, 1, 16384));
    unsigned long long* const dst_n = recorder_counter(dst, kind);
    if (kind == HML_REC_LEVELS)
        hipLaunchKernelGGL(hml_k_rec_merge_list<double>, grid, dim3(256), 0, dst->stream, d_pos, (const double*)cells, (uint32_t)M, (uint32_t)T, (int)rows, (unsigned long long)N, rd.acc<double>(), rd.d_boundary, dst_n);
    else if (kind == HML_REC_BREAKS)
        hipLaunchKernelGGL(hml_k_rec_merge_list<uint32_t>, grid, dim3(256), 0, dst->stream, d_pos, (const uint32_t*)cells, (uint32_t)M, (uint32_t)T, (int)rows, (unsigned long long)N, rd.acc<uint32_t>(), rd.d_boundary, dst_n);
    else
        hipLaunchKernelGGL(hml_k_rec_merge_list<int32_t>, grid, dim3(256), 0, dst->stream, d_pos, (const int32_t*)cells, (uint32_t)M, (uint32_t)T, (int)rows, (unsigned long long)N, rd.acc<int32_t>(), rd.d_boundary, dst_n);
    KLAUNCH_CHECK();
    HIPCHK(hipStreamSynchronize(dst->stream));
    return 0;
}

extern "C" {

int hml_recording_payload_size(hml_ctx* c, int kind, uint64_t* n_bytes) {
    NEED_MODEL();
    if (!n_bytes) return set_err(HML_ERR_ARG, "null argument");
    if (int r = payload_kind(kind)) return r;
    uint64_t M = 0;
    DevBuf b_seg;
    const uint32_t* d_pos = nullptr;
    if (int r = payload_positions(c, kind, &M, b_seg, &d_pos)) return r;
    *n_bytes = payload_bytes(M, (uint64_t)recorder_rows(c, kind), hml_recorder_kinds[kind].elem);
    return 0;
}

int hml_recording_export(hml_ctx* c, int kind, void* payload_dev, uint64_t capacity_bytes, uint64_t* n_bytes) {
    NEED_MODEL();
    if (int r = payload_kind(kind)) return r;
    return payload_export(c, kind, payload_dev, capacity_bytes, n_bytes);
}

int hml_recording_merge_payload(hml_ctx* dst, int kind, const void* payload_dev, uint64_t n_bytes) { return payload_merge(dst, kind, payload_dev, n_bytes); }

int hml_recording_merge_across(hml_ctx* dst, hml_ctx* src, int kind) {
    if (!dst || !src || !dst->model_set || !src->model_set) return set_err(HML_ERR_ARG, "model not set");
    if (int r = payload_kind(kind)) return r;
    const hml_recorder_kind& rk = hml_recorder_kinds[kind];
    const bool per_dimension = kind != HML_REC_BREAKS;
    if (dst == src) return set_err(HML_ERR_ARG, "a context cannot be merged into itself");
    if (dst->T != src->T || (per_dimension && dst->D != src->D))
        return set_err(HML_ERR_ARG, std::string(rk.noun) + " can only be merged between chains over the same positions" + (per_dimension ? " and dimensions" : ""));
    if (!src->rec[kind].asked) return recorder_none(kind, "the source");
    // the export, on the source's device
    if (int r = ctx_bind(src)) return r;
    if (int r = settle_if_limited(src)) return r;
    uint64_t bytes = 0;
    DevBuf b_src, b_dst;
    {
        uint64_t M = 0;
        DevBuf b_seg;
        const uint32_t* d_pos = nullptr;
        if (int r = payload_positions(src, kind, &M, b_seg, &d_pos)) return r;
        bytes = payload_bytes(M, (uint64_t)recorder_rows(src, kind), rk.elem);
    }
    HIPCHK(b_src.alloc(bytes));
    uint64_t written = 0;
    if (int r = payload_export(src, kind, b_src.get(), bytes, &written)) return r;
    if (written != bytes) return set_err(HML_ERR_HIP, "internal error: a recording changed between its sizing and its export");
    if (dst->device == src->device) return payload_merge(dst, kind, b_src.get(), bytes);
    // ... its bytes to the destination's device (no peer access needed), and the merge there
    if (int r = ctx_bind(dst)) return r;
    HIPCHK(b_dst.alloc(bytes));
    HIPCHK(hipMemcpyPeer(b_dst.get(), dst->device, b_src.get(), src->device, bytes));
    HIPCHK(hipDeviceSynchronize());
    return payload_merge(dst, kind, b_dst.get(), bytes);
}

}  // extern "C"

// ---------------------------------------------------------------------------------------- history (hml_k_history.h)
// A row of scalars per due sweep, written on the device behind the sweep's parameter update.  The host only makes room ahead
// of the sweeps it enqueues, and reads the rows when asked.
#include "hml_k_history.h"   // (launched from this object alone)
#include "hml_history_stats.h"

static_assert(HML_HIST_COLS == HML_HISTORY_COLS, "the kernel's row and the C ABI's");
static const char* const hml_history_columns[HML_HISTORY_COLS] = {"sweep", "method", "ll_emit", "ll_path", "lprior_theta", "lprior_path",
                                                                  "segments", "blocks", "states_used", "threshold", "chain"};
static uint64_t history_bytes(uint64_t cap) { return sizeof(hml_history_head) + cap * HML_HISTORY_COLS * sizeof(double); }

// the buffer's head as the device holds it (the context's device is current; the caller has settled the chain)
static int history_head(hml_ctx* c, hml_history_head* h) {
    memset(h, 0, sizeof *h);
    if (!c->hist.d_buf) return 0;
    HIPCHK(hipMemcpyAsync(h, c->hist.d_buf.get(), sizeof *h, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

// Room for the rows of `iterations` further sweeps: rows present + iterations / every + 1, at least.  `expected` counts the
// rows the sweeps enqueued so far will have left (the chain's sweep counter is `requested` once they have run), so a call that
// finds room adds no synchronisation.  Without room the stream is waited for, the count is taken from the device, and a
// buffer of twice the size (or what is needed) takes the rows over, device to device; the captured graph holds the old one.
int hml_history_ensure(hml_ctx* c, uint64_t iterations) {
    hml_history& hs = c->hist;
    if (!hs.on) return 0;
    const uint64_t every = hs.every ? hs.every : 1;
    const uint64_t due = (c->requested + iterations) / every - c->requested / every;
    if (hs.d_buf && hs.expected + iterations / every + 1 <= hs.cap) { hs.expected += due; return 0; }
    hml_history_head head;
    memset(&head, 0, sizeof head);
    if (hs.d_buf) {
        HIPCHK(hipStreamSynchronize(c->stream));
        // (a halted chain's skipped sweeps run again later and write behind what is there: they are counted in `expected`)
        if (!chain_halted(c)) {
            if (int r = history_head(c, &head)) return r;
            hs.expected = head.n_rows;
            if (hs.expected + iterations / every + 1 <= hs.cap) { hs.expected += due; return 0; }
        }
    }
    const uint64_t need = hs.expected + iterations / every + 1;
    const uint64_t cap = std::max<uint64_t>(std::max<uint64_t>(2 * hs.cap, need), 16);
    DevBuf nb;
    HIPCHK(nb.alloc(history_bytes(cap)));
    if (hs.d_buf) HIPCHK(hipMemcpyAsync(nb.get(), hs.d_buf.get(), history_bytes(hs.cap), hipMemcpyDeviceToDevice, c->stream));
    else HIPCHK(hipMemsetAsync(nb.get(), 0, sizeof(hml_history_head), c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));   // (chains batched by hml_iterate_many run on their group's stream; the old buffer goes below)
    if (hs.d_buf) hs.grown++;
    hs.d_buf.swap(nb);
    hs.cap = cap;
    hs.expected += due;
    drop_graph(c);
    return 0;
}

void hml_history_launch(hml_ctx* c, hipStream_t s, char method) {
    hipLaunchKernelGGL(hml_k_history, dim3(1), dim3(64), 0, s, c->d_mdl.get(), c->d_q.get(), c->hist.d_buf.as<hml_history_head>(),
                       (unsigned long long)c->hist.cap, (unsigned long long)(c->hist.every ? c->hist.every : 1), method == HML_METHOD_MIXTURE ? 1 : 0, c->chain);
}

// every row of a context, on the host
static int history_fetch(hml_ctx* c, std::vector<double>& rows, uint64_t* n_rows, uint64_t* n_dropped) {
    if (!c) return set_err(HML_ERR_ARG, "null context");
    rows.clear();
    *n_rows = 0;
    if (n_dropped) *n_dropped = 0;
    if (!c->hist.d_buf) return 0;
    if (int r = ctx_bind(c)) return r;
    if (int r = hml_settle(c)) return r;
    hml_history_head head;
    if (int r = history_head(c, &head)) return r;
    const uint64_t n = std::min<uint64_t>(head.n_rows, c->hist.cap);
    rows.resize(n * HML_HISTORY_COLS);
    if (n) HIPCHK(hipMemcpy(rows.data(), c->hist.d_buf.as<char>() + sizeof(hml_history_head), n * HML_HISTORY_COLS * sizeof(double), hipMemcpyDeviceToHost));
    *n_rows = n;
    if (n_dropped) *n_dropped = head.dropped;
    return 0;
}

extern "C" {

int hml_set_history(hml_ctx* c, int on, uint64_t every) {
    if (!c) return set_err(HML_ERR_ARG, "null context");
    if (on && every < 1) return set_err(HML_ERR_ARG, "hml_set_history: every must be at least 1");
    if (c->model_set || c->graph_exec) {
        if (int r = ctx_bind(c)) return r;
        // (sweeps a halted chain skipped run again under the setting they were enqueued with)
        if (c->model_set) { if (int r = settle_if_limited(c)) return r; }
        drop_graph(c);   // a captured sweep holds the launch, or lacks it
    }
    c->hist.on = on != 0;
    if (on) c->hist.every = every;
    return 0;
}

int hml_history_size(hml_ctx* c, uint64_t* n_rows, uint64_t* n_dropped) {
    if (!c) return set_err(HML_ERR_ARG, "null context");
    if (n_rows) *n_rows = 0;
    if (n_dropped) *n_dropped = 0;
    if (!c->hist.d_buf) return 0;
    if (int r = ctx_bind(c)) return r;
    if (int r = hml_settle(c)) return r;
    hml_history_head head;
    if (int r = history_head(c, &head)) return r;
    if (n_rows) *n_rows = std::min<uint64_t>(head.n_rows, c->hist.cap);
    if (n_dropped) *n_dropped = head.dropped;
    return 0;
}

int hml_history_read(hml_ctx* c, uint64_t first, uint64_t n, double* rows) {
    if (!c) return set_err(HML_ERR_ARG, "null context");
    if (n == 0) return 0;
    if (!rows) return set_err(HML_ERR_ARG, "null argument");
    uint64_t have = 0;
    if (int r = hml_history_size(c, &have, nullptr)) return r;
    if (first > have || n > have - first) return set_err(HML_ERR_ARG, "hml_history_read: rows beyond the " + std::to_string(have) + " the history holds");
    HIPCHK(hipMemcpy(rows, c->hist.d_buf.as<char>() + sizeof(hml_history_head) + first * HML_HISTORY_COLS * sizeof(double), n * HML_HISTORY_COLS * sizeof(double),
                     hipMemcpyDeviceToHost));
    return 0;
}

int hml_history_clear(hml_ctx* c) {
    if (!c) return set_err(HML_ERR_ARG, "null context");
    c->hist.expected = 0;
    if (!c->hist.d_buf) return 0;
    if (int r = ctx_bind(c)) return r;
    if (int r = hml_settle(c)) return r;
    HIPCHK(hipMemsetAsync(c->hist.d_buf.get(), 0, sizeof(hml_history_head), c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

const char* hml_history_column(int col) { return col >= 0 && col < HML_HISTORY_COLS ? hml_history_columns[col] : nullptr; }

int hml_history_stats(const double* x, int n_chains, uint64_t n, double* rhat, double* ess, double* chain_mean, double* chain_sd, uint64_t* n_nonfinite) {
    const char* why = nullptr;
    if (hml_history_stats_compute(x, n_chains, n, rhat, ess, chain_mean, chain_sd, n_nonfinite, &why)) return set_err(HML_ERR_ARG, why ? why : "history statistics");
    return 0;
}

int hml_history_summary(hml_ctx* const* ctxs, int n, int col, uint64_t skip_sweeps, double* rhat, double* ess, double* chain_mean, double* chain_sd,
                        uint64_t* n_used, uint64_t* n_nonfinite) {
    if (!ctxs || n < 1) return set_err(HML_ERR_ARG, "no contexts");
    if (!((col >= 0 && col < HML_HISTORY_COLS) || col == HML_HISTORY_LOGLIK || col == HML_HISTORY_LOGPOST))
        return set_err(HML_ERR_ARG, "hml_history_summary: a column 0 ... 10, HML_HISTORY_LOGLIK or HML_HISTORY_LOGPOST");
    std::vector<std::vector<double>> series((size_t)n);
    uint64_t used = ~0ull;
    for (int k = 0; k < n; ++k) {
        std::vector<double> rows;
        uint64_t have = 0;
        if (int r = history_fetch(ctxs[k], rows, &have, nullptr)) return r;
        for (uint64_t i = 0; i < have; ++i) {
            const double* row = rows.data() + i * HML_HISTORY_COLS;
            if (!(row[0] > (double)skip_sweeps)) continue;
            series[k].push_back(col == HML_HISTORY_LOGLIK ? row[2] + row[3] : col == HML_HISTORY_LOGPOST ? ((row[2] + row[3]) + row[4]) + row[5] : row[col]);
        }
        used = std::min<uint64_t>(used, series[k].size());
    }
    if (n_used) *n_used = used;
    std::vector<double> x((size_t)n * used);
    for (int k = 0; k < n; ++k) std::copy(series[k].end() - (ptrdiff_t)used, series[k].end(), x.begin() + (ptrdiff_t)((uint64_t)k * used));
    return hml_history_stats(x.data(), n, used, rhat, ess, chain_mean, chain_sd, n_nonfinite);
}

}  // extern "C"

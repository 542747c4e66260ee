// libhammlet_hip.so - the read-outs of the C ABI (include/hml.h): what the recorded sweeps accumulated per position - state
// marginals, emission levels, breakpoints, level bands - brought into the forms the callers ask for, and the merges of one
// chain's recording into another's: on one device from recorder to recorder, across devices through the sparse payload of
// hml_k_rec_payload.h.  Nothing here runs inside a sweep; hml_capi.hip holds the chain itself.
#define HML_REGIONS_KERNELS   // (hml_k_regions.h: this object holds the regions' kernels)
#include "hml_capi_shared.hpp"
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

// The fixed-shape scan of hml_k_scan.h over `rows` rows of M entries on stream `s`: inclusive into d_out[rows][M] (d_out may
// be d_in), or exclusive into d_out[rows][M + 1] with the totals last.
template <typename In, typename Acc, bool Exclusive>
static int scan_rows(hipStream_t s, const In* d_in, uint64_t M, int rows, Acc* d_out) {
    DevBuf d_cs;
    const uint32_t n_chunks = (uint32_t)((M + HML_SCAN_CHUNK - 1) / HML_SCAN_CHUNK);
    HIPCHK(d_cs.alloc(((uint64_t)n_chunks * rows + 1) * sizeof(Acc)));
    const dim3 grid((unsigned)grid_for(n_chunks, 1, 1, 4096), (unsigned)rows);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_k_scan_partial<In, Acc>), grid, dim3(256), 0, s, d_in, (uint32_t)M, n_chunks, d_cs.as<Acc>());
    hipLaunchKernelGGL(hml_k_scan_chunks<Acc>, dim3(rows), dim3(1024), 0, s, d_cs.as<Acc>(), n_chunks);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_k_scan_final<In, Acc, Exclusive>), grid, dim3(256), 0, s, d_in, (uint32_t)M, n_chunks, (const Acc*)d_cs.as<Acc>(), d_out);
    KLAUNCH_CHECK();
    HIPCHK(hipStreamSynchronize(s));   // (d_cs goes with this frame)
    return 0;
}

static int model_fault(const hml_model& m) {   // the device error a sweep left in the model, if any
    if (!m.err_code) return 0;
    char buf[256];
    return set_err(HML_ERR_MODEL, deverr_text(m.err_code, m.err_value, buf, sizeof buf));
}

// M ascending starts (the first is position 0) and T into the M lengths
static void lengths_of(const uint32_t* start, uint64_t M, uint32_t T, uint64_t* len) {
    for (uint64_t i = 0; i < M; ++i) len[i] = (uint64_t)((i + 1 < M ? start[i + 1] : T) - start[i]);
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
    DevBuf b_seg, b_g, b_cs, b_rc, b_key;
    if (int r = table_segments(c, tab, &M, b_seg, b_g)) return r;
    const uint32_t n_chunks = (uint32_t)((M + 255) / 256);
    HIPCHK(b_cs.alloc((uint64_t)ncol * n_chunks * sizeof(int32_t)));
    HIPCHK(b_rc.alloc(((uint64_t)n_chunks + 1) * sizeof(int32_t)));
    HIPCHK(b_key.alloc(M * sizeof(int16_t)));
    int32_t *const d_cs = b_cs.as<int32_t>(), *const d_rc = b_rc.as<int32_t>();
    int16_t* const d_key = b_key.as<int16_t>();
    HIPCHK(hipMemsetAsync(d_rc + n_chunks, 0, sizeof(int32_t), c->stream));
    hipLaunchKernelGGL(hml_k_seg_partial, dim3(n_chunks), dim3(256), 0, c->stream, b_g.as<int32_t>(), (uint32_t)M, ncol, d_cs, n_chunks);
    hipLaunchKernelGGL(hml_k_scan_chunks<int32_t>, dim3(ncol), dim3(1024), 0, c->stream, d_cs, n_chunks);
    pick(b_g.as<int32_t>(), (uint32_t)M, d_cs, n_chunks, d_key);
    hipLaunchKernelGGL(hml_k_seg_run_count, dim3(n_chunks), dim3(256), 0, c->stream, d_key, (uint32_t)M, d_rc);
    hipLaunchKernelGGL(hml_k_scan_chunks<int32_t>, dim3(1), dim3(1024), 0, c->stream, d_rc, n_chunks + 1u);   // d_rc[n_chunks] = total
    KLAUNCH_CHECK();
    int32_t R = 0;
    HIPCHK(hipMemcpyAsync(&R, d_rc + n_chunks, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    *n_runs = (uint64_t)R;
    if (!run_len) return 0;
    DevBuf b_rs, b_rq;
    HIPCHK(b_rs.alloc((uint64_t)R * sizeof(uint32_t)));
    HIPCHK(b_rq.alloc((uint64_t)R * sizeof(int16_t)));
    hipLaunchKernelGGL(hml_k_seg_run_scatter, dim3(n_chunks), dim3(256), 0, c->stream, d_key, b_seg.as<uint32_t>(), (uint32_t)M, d_rc, b_rs.as<uint32_t>(), b_rq.as<int16_t>());
    KLAUNCH_CHECK();
    std::vector<uint32_t> h_rs(R);
    run_key.resize(R);
    HIPCHK(hipMemcpyAsync(h_rs.data(), b_rs.get(), (uint64_t)R * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(run_key.data(), b_rq.get(), (uint64_t)R * sizeof(int16_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    lengths_of(h_rs.data(), (uint64_t)R, (uint32_t)c->T, run_len);
    return 0;
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

// ---------------------------------------------------------------------------------------- Viterbi decode (hml_k_viterbi.h)
// The jointly most probable state path over the current blocks under the current parameters.  Everything a decode allocates
// is local to the call: it goes on every path out, and the context keeps only the numbers of hml_viterbi_info.
#include "hml_k_viterbi.h"   // (launched from this object alone)

struct vit_tables { DevBuf par, trans, init; };
struct vit_path { DevBuf q; long long score = 0; uint32_t B = 0; };

// the launches templated on the states the recursion's vector is kept for
template <int KM>
static void vit_launch_forward(hml_ctx* c, const vit_tables& t, uint32_t L, uint32_t W, uint32_t n_chunks, long long* entry, long long* exitv, uint8_t* psi) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_k_vit_forward<KM>), dim3((n_chunks + 63u) / 64u), dim3(64), 0, c->stream, t.par.as<hml_vit_par>(), t.trans.as<long long>(),
                       t.init.as<long long>(), c->d_ia, c->d_starts.get(), L, W, n_chunks, entry, exitv, psi);
}
template <int KM>
static void vit_launch_rerun(hml_ctx* c, const vit_tables& t, uint32_t L, uint32_t n_chunks, const uint32_t* heads, uint32_t n_heads, const uint8_t* match, long long* entry,
                             long long* exitv, uint8_t* psi) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_k_vit_rerun<KM>), dim3((n_heads + 63u) / 64u), dim3(64), 0, c->stream, t.par.as<hml_vit_par>(), t.trans.as<long long>(),
                       t.init.as<long long>(), c->d_ia, c->d_starts.get(), L, n_chunks, heads, n_heads, match, entry, exitv, psi);
}
template <int KM>
static void vit_launch_finish(hml_ctx* c, const vit_tables& t, uint32_t L, uint32_t n_chunks, const uint8_t* match, long long* entry, long long* exitv, uint8_t* psi,
                              unsigned long long* walked) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_k_vit_finish<KM>), dim3(1), dim3(64), 0, c->stream, t.par.as<hml_vit_par>(), t.trans.as<long long>(), t.init.as<long long>(),
                       c->d_ia, c->d_starts.get(), L, n_chunks, match, entry, exitv, psi, walked);
}
#define VIT_BY_K(K, fn, ...) do { if ((K) <= 8) fn<8>(__VA_ARGS__); else if ((K) <= 16) fn<16>(__VA_ARGS__); else fn<HML_CAP_K>(__VA_ARGS__); } while (0)

// how a decode begins: a settled chain with blocks, and the tables (parameters, trans, init) on the device
static int vit_begin(hml_ctx* c, vit_tables& t, uint32_t* B_out) {
    hml_model m; if (int r = fetch_model(c, &m)) return r;
    if (int r = model_fault(m)) return r;
    if (m.halted) return set_err(HML_ERR_ARG, "hml_viterbi: the chain is halted; settle it with hml_sync first");
    if (m.B == 0) return set_err(HML_ERR_ARG, "hml_viterbi: no blocks yet: run a sweep or hml_create_blocks first");
    const int K = c->K;
    HIPCHK(t.par.alloc(sizeof(hml_vit_par)));
    HIPCHK(t.trans.alloc((uint64_t)K * K * sizeof(long long)));
    HIPCHK(t.init.alloc((uint64_t)K * sizeof(long long)));
    hipLaunchKernelGGL(hml_k_vit_tables, dim3(1), dim3(256), 0, c->stream, c->d_mdl.get(), t.par.as<hml_vit_par>(), t.trans.as<long long>(), t.init.as<long long>());
    KLAUNCH_CHECK();
    *B_out = m.B;
    return 0;
}

// the decode: path (device, int16 per block) and score
static int vit_decode(hml_ctx* c, vit_path& out) {
    vit_tables t;
    uint32_t B = 0;
    if (int r = vit_begin(c, t, &B)) return r;
    const int K = c->K;
    const uint32_t L = c->vit.L ? c->vit.L : HML_VIT_DEFAULT_L;
    const uint32_t W = c->vit.W ? c->vit.W : HML_VIT_DEFAULT_W;
    const uint32_t n_chunks = (uint32_t)(((uint64_t)B + L - 1u) / L);
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
    long long *const entry = b_entry.as<long long>(), *const exitv = b_exit.as<long long>();
    uint8_t *const psi = b_psi.as<uint8_t>(), *const match = b_match.as<uint8_t>();
    uint32_t* const list = b_list.as<uint32_t>();
    unsigned long long* const words = b_words.as<unsigned long long>();
    HIPCHK(hipMemsetAsync(words, 0, 4 * sizeof(unsigned long long), c->stream));

    VIT_BY_K(K, vit_launch_forward, c, t, L, W, n_chunks, entry, exitv, psi);
    KLAUNCH_CHECK();
    // verify; repair in rounds while chunks are stale; the single lane for what the rounds leave
    uint32_t n_stale = 0, stale_first = 0, rounds_run = 0;
    unsigned long long walked = 0;
    for (uint32_t round = 0;; ++round) {
        uint32_t h_cnt[2] = {0, 0};   // stale chunks, heads of their runs
        HIPCHK(hipMemsetAsync(words, 0, sizeof h_cnt, c->stream));
        hipLaunchKernelGGL(hml_k_vit_verify, dim3(grid_for(n_chunks, 256, 1, 4096)), dim3(256), 0, c->stream, entry, exitv, K, n_chunks, match, list, (uint32_t*)words,
                           (uint32_t*)words + 1);
        KLAUNCH_CHECK();
        HIPCHK(hipMemcpyAsync(h_cnt, words, sizeof h_cnt, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        n_stale = h_cnt[0];
        if (round == 0) stale_first = n_stale;
        if (n_stale == 0 || round >= c->vit.rounds) break;
        VIT_BY_K(K, vit_launch_rerun, c, t, L, n_chunks, list, h_cnt[1], match, entry, exitv, psi);
        KLAUNCH_CHECK();
        rounds_run = round + 1u;
    }
    if (n_stale) {
        VIT_BY_K(K, vit_launch_finish, c, t, L, n_chunks, match, entry, exitv, psi, words + 1);
        KLAUNCH_CHECK();
    }
    // back-track
    const dim3 cgrid((n_chunks + 63u) / 64u), ggrid((n_groups + 63u) / 64u);
    hipLaunchKernelGGL(hml_k_vit_chunk_maps, cgrid, dim3(64), 0, c->stream, psi, K, B, L, n_chunks, b_maps.as<uint8_t>());
    hipLaunchKernelGGL(hml_k_vit_group_maps, ggrid, dim3(64), 0, c->stream, b_maps.as<uint8_t>(), K, n_chunks, S, n_groups, b_gmaps.as<uint8_t>());
    hipLaunchKernelGGL(hml_k_vit_group_ends, dim3(1), dim3(64), 0, c->stream, exitv, b_gmaps.as<uint8_t>(), K, n_chunks, n_groups, b_gend.as<uint8_t>());
    hipLaunchKernelGGL(hml_k_vit_chunk_ends, ggrid, dim3(64), 0, c->stream, b_maps.as<uint8_t>(), b_gend.as<uint8_t>(), K, n_chunks, S, n_groups, b_cend.as<uint8_t>());
    hipLaunchKernelGGL(hml_k_vit_walk, cgrid, dim3(64), 0, c->stream, psi, b_cend.as<uint8_t>(), K, B, L, n_chunks, out.q.as<int16_t>());
    hipLaunchKernelGGL(hml_k_vit_score, dim3(grid_for(B, 256, 1, 4096)), dim3(256), 0, c->stream, t.par.as<hml_vit_par>(), t.trans.as<long long>(), t.init.as<long long>(),
                       c->d_ia, c->d_starts.get(), out.q.as<int16_t>(), words + 2);
    KLAUNCH_CHECK();
    unsigned long long h_words[4];
    HIPCHK(hipMemcpyAsync(h_words, words, sizeof h_words, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));   // (the scratch goes with this frame)
    walked = h_words[1];
    out.score = (long long)h_words[2];
    out.B = B;
    c->vit.decoded = true;
    c->vit.chunks = n_chunks; c->vit.used_L = L; c->vit.used_W = W; c->vit.stale = stale_first; c->vit.rounds_run = rounds_run; c->vit.walked = walked;
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
    // runs of equal state over the blocks: the flag / count / scatter steps of the segmentation read-out, on block starts
    const uint32_t M = p.B;
    const uint32_t n_chunks = (M + 255u) / 256u;
    DevBuf b_rc, b_rs, b_rq;
    HIPCHK(b_rc.alloc(((uint64_t)n_chunks + 1) * sizeof(int32_t)));
    int32_t* const d_rc = b_rc.as<int32_t>();
    HIPCHK(hipMemsetAsync(d_rc + n_chunks, 0, sizeof(int32_t), c->stream));
    hipLaunchKernelGGL(hml_k_seg_run_count, dim3(n_chunks), dim3(256), 0, c->stream, p.q.as<int16_t>(), M, d_rc);
    hipLaunchKernelGGL(hml_k_scan_chunks<int32_t>, dim3(1), dim3(1024), 0, c->stream, d_rc, n_chunks + 1u);   // d_rc[n_chunks] = total
    KLAUNCH_CHECK();
    int32_t R = 0;
    HIPCHK(hipMemcpyAsync(&R, d_rc + n_chunks, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    *n_runs = (uint64_t)R;
    if (!run_len) return 0;
    HIPCHK(b_rs.alloc((uint64_t)R * sizeof(uint32_t)));
    HIPCHK(b_rq.alloc((uint64_t)R * sizeof(int16_t)));
    hipLaunchKernelGGL(hml_k_seg_run_scatter, dim3(n_chunks), dim3(256), 0, c->stream, p.q.as<int16_t>(), c->d_starts.get(), M, d_rc, b_rs.as<uint32_t>(), b_rq.as<int16_t>());
    KLAUNCH_CHECK();
    std::vector<uint32_t> h_rs(R);
    std::vector<int16_t> h_rq(R);
    HIPCHK(hipMemcpyAsync(h_rs.data(), b_rs.get(), (uint64_t)R * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(h_rq.data(), b_rq.get(), (uint64_t)R * sizeof(int16_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    lengths_of(h_rs.data(), (uint64_t)R, (uint32_t)c->T, run_len);
    if (run_state) std::copy(h_rq.begin(), h_rq.end(), run_state);
    return 0;
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
    vit_tables t;
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
    if (!c->vit.decoded) return set_err(HML_ERR_ARG, "hml_viterbi_info: nothing was decoded yet");
    if (chunks) *chunks = c->vit.chunks;
    if (L) *L = c->vit.used_L;
    if (W) *W = c->vit.used_W;
    if (stale_chunks) *stale_chunks = c->vit.stale;
    if (rounds) *rounds = c->vit.rounds_run;
    if (serial_chunks) *serial_chunks = c->vit.walked;
    return 0;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------- smoothing (hml_k_posterior.h)
// State posteriors per block, log p(y | theta) and the call with a confidence per run: the sum-product sibling of the decode
// above, with the same relation to the chain (read only) and to device memory (all of it local to the call).
#include "hml_k_posterior.h"   // (launched from this object alone)

struct post_tables { DevBuf par, A, pi; };
struct post_result {
    DevBuf gamma, q, conf, alpha, cval, beta;   // gamma only if asked for
    double loglik = 0.0;
    uint64_t degenerate = 0;
    uint32_t B = 0;
};

template <int KM, int DIR>
static void post_launch_first(hml_ctx* c, const hml_post_args& a, size_t lds) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_k_post_first<KM, DIR>), dim3((a.n_chunks + 63u) / 64u), dim3(64), lds, c->stream, a);
}
template <int KM, int DIR>
static void post_launch_rerun(hml_ctx* c, const hml_post_args& a, size_t lds, const uint32_t* heads, uint32_t n_heads, const uint8_t* match) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_k_post_rerun<KM, DIR>), dim3((n_heads + 63u) / 64u), dim3(64), lds, c->stream, a, heads, n_heads, match);
}
template <int KM, int DIR>
static void post_launch_finish(hml_ctx* c, const hml_post_args& a, size_t lds, const uint8_t* match, unsigned long long* walked) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_k_post_finish<KM, DIR>), dim3(1), dim3(64), lds, c->stream, a, match, walked);
}
#define POST_BY_K(K, DIR, fn, ...) do { if ((K) <= 8) fn<8, DIR>(__VA_ARGS__); else if ((K) <= 16) fn<16, DIR>(__VA_ARGS__); else fn<HML_CAP_K, DIR>(__VA_ARGS__); } while (0)

// how a call begins: a settled chain with blocks, and the tables (parameters, A and pi in double) on the device
static int post_ready(const hml_model& m) {
    if (int r = model_fault(m)) return r;
    if (m.halted) return set_err(HML_ERR_ARG, "hml_posterior: the chain is halted; settle it with hml_sync first");
    if (m.B == 0) return set_err(HML_ERR_ARG, "hml_posterior: no blocks yet: run a sweep or hml_create_blocks first");
    return 0;
}
static int post_begin(hml_ctx* c, post_tables& t, uint32_t* B_out) {
    hml_model m; if (int r = fetch_model(c, &m)) return r;
    if (int r = post_ready(m)) return r;
    const int K = c->K;
    HIPCHK(t.par.alloc(sizeof(hml_vit_par)));
    HIPCHK(t.A.alloc((uint64_t)K * K * sizeof(double)));
    HIPCHK(t.pi.alloc((uint64_t)K * sizeof(double)));
    hipLaunchKernelGGL(hml_k_post_tables, dim3(1), dim3(256), 0, c->stream, c->d_mdl.get(), t.par.as<hml_vit_par>(), t.A.as<double>(), t.pi.as<double>());
    KLAUNCH_CHECK();
    *B_out = m.B;
    return 0;
}

// one direction: first run, then verify / repair in rounds / the single lane, as vit_decode does it
template <int DIR>
static int post_direction(hml_ctx* c, const hml_post_args& a, int K, uint8_t* match, uint32_t* list, unsigned long long* words, uint64_t* stale_first_out,
                          uint64_t* rounds_out, bool* finished_out) {
    const size_t lds = ((size_t)K * K + K) * sizeof(double);
    POST_BY_K(K, DIR, post_launch_first, c, a, lds);
    KLAUNCH_CHECK();
    uint32_t n_stale = 0;
    uint64_t rounds_run = 0;
    for (uint32_t round = 0;; ++round) {
        uint32_t h_cnt[2] = {0, 0};   // stale chunks, heads of their runs
        HIPCHK(hipMemsetAsync(words, 0, sizeof h_cnt, c->stream));
        hipLaunchKernelGGL(hml_k_vit_verify, dim3(grid_for(a.n_chunks, 256, 1, 4096)), dim3(256), 0, c->stream, reinterpret_cast<const long long*>(a.entry),
                           reinterpret_cast<const long long*>(a.exitv), K, a.n_chunks, match, list, (uint32_t*)words, (uint32_t*)words + 1);
        KLAUNCH_CHECK();
        HIPCHK(hipMemcpyAsync(h_cnt, words, sizeof h_cnt, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        n_stale = h_cnt[0];
        if (round == 0) *stale_first_out = n_stale;
        if (n_stale == 0 || round >= c->post.rounds) break;
        POST_BY_K(K, DIR, post_launch_rerun, c, a, lds, list, h_cnt[1], match);
        KLAUNCH_CHECK();
        rounds_run = round + 1u;
    }
    if (n_stale) {
        POST_BY_K(K, DIR, post_launch_finish, c, a, lds, match, words + 1);
        KLAUNCH_CHECK();
    }
    *rounds_out = rounds_run;
    *finished_out = n_stale != 0;
    return 0;
}

// the whole computation; the rows alpha, c and beta stay in `out` for the probe, the tables in `t` for the E-step
static int post_compute(hml_ctx* c, bool want_gamma, post_result& out, post_tables& t) {
    uint32_t B = 0;
    if (int r = post_begin(c, t, &B)) return r;
    const int K = c->K;
    const uint32_t L = c->post.L ? c->post.L : HML_POST_DEFAULT_L;
    const uint32_t W = c->post.W ? c->post.W : HML_POST_DEFAULT_W;
    const uint32_t n_chunks = (uint32_t)(((uint64_t)B + L - 1u) / L);
    const uint64_t n1 = ((uint64_t)B + 63u) / 64u, n2 = (n1 + 63u) / 64u;   // the first two levels of the tree
    DevBuf b_entry, b_exit, b_match, b_list, b_words, b_ell, b_t1, b_t2;
    HIPCHK(out.alpha.alloc((uint64_t)B * K * sizeof(double)));
    HIPCHK(out.beta.alloc((uint64_t)B * K * sizeof(double)));
    HIPCHK(out.cval.alloc((uint64_t)B * sizeof(double)));
    HIPCHK(b_ell.alloc((uint64_t)B * sizeof(double)));
    HIPCHK(b_entry.alloc((uint64_t)n_chunks * K * sizeof(double)));
    HIPCHK(b_exit.alloc((uint64_t)n_chunks * K * sizeof(double)));
    HIPCHK(b_match.alloc(n_chunks));
    HIPCHK(b_list.alloc((uint64_t)n_chunks * sizeof(uint32_t)));
    HIPCHK(b_words.alloc(4 * sizeof(unsigned long long)));   // [0] stale chunks and heads (32 bits each), [1] chunks the single lane ran, [2] degenerate blocks, [3] log-likelihood
    HIPCHK(b_t1.alloc(n1 * sizeof(double)));
    HIPCHK(b_t2.alloc(n2 * sizeof(double)));
    HIPCHK(out.q.alloc((uint64_t)B * sizeof(int16_t)));
    HIPCHK(out.conf.alloc((uint64_t)B * sizeof(double)));
    if (want_gamma) HIPCHK(out.gamma.alloc((uint64_t)B * K * sizeof(double)));
    unsigned long long* const words = b_words.as<unsigned long long>();
    HIPCHK(hipMemsetAsync(words, 0, 4 * sizeof(unsigned long long), c->stream));

    hml_post_args a;
    a.par = t.par.as<hml_vit_par>(); a.A = t.A.as<double>(); a.pi = t.pi.as<double>();
    a.ia = c->d_ia; a.starts = c->d_starts.get();
    a.L = L; a.W = W; a.n_chunks = n_chunks;
    a.entry = b_entry.as<double>(); a.exitv = b_exit.as<double>();
    uint64_t stale[2] = {0, 0}, rounds[2] = {0, 0};
    bool finished[2] = {false, false};
    a.rows = out.alpha.as<double>(); a.cval = out.cval.as<double>(); a.ell = b_ell.as<double>();
    if (int r = post_direction<0>(c, a, K, b_match.as<uint8_t>(), b_list.as<uint32_t>(), words, &stale[0], &rounds[0], &finished[0])) return r;
    a.rows = out.beta.as<double>(); a.cval = nullptr; a.ell = nullptr;   // (entry, exit, match and list are used again)
    if (int r = post_direction<1>(c, a, K, b_match.as<uint8_t>(), b_list.as<uint32_t>(), words, &stale[1], &rounds[1], &finished[1])) return r;

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
    c->post.computed = true;
    c->post.chunks = n_chunks; c->post.used_L = L; c->post.used_W = W; c->post.stale_fwd = stale[0]; c->post.stale_bwd = stale[1];
    c->post.rounds_run = std::max(rounds[0], rounds[1]); c->post.walked = (finished[0] || finished[1]) ? h_words[1] : 0;
    return 0;
}

static int post_compute(hml_ctx* c, bool want_gamma, post_result& out) {
    post_tables t;
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
    const uint32_t M = p.B;
    const uint32_t n_chunks = (M + 255u) / 256u;
    DevBuf b_rc, b_rs, b_rq, b_rconf;
    HIPCHK(b_rc.alloc(((uint64_t)n_chunks + 1) * sizeof(int32_t)));
    int32_t* const d_rc = b_rc.as<int32_t>();
    HIPCHK(hipMemsetAsync(d_rc + n_chunks, 0, sizeof(int32_t), c->stream));
    hipLaunchKernelGGL(hml_k_seg_run_count, dim3(n_chunks), dim3(256), 0, c->stream, p.q.as<int16_t>(), M, d_rc);
    hipLaunchKernelGGL(hml_k_scan_chunks<int32_t>, dim3(1), dim3(1024), 0, c->stream, d_rc, n_chunks + 1u);   // d_rc[n_chunks] = total
    KLAUNCH_CHECK();
    int32_t R = 0;
    HIPCHK(hipMemcpyAsync(&R, d_rc + n_chunks, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    *n_runs = (uint64_t)R;
    if (!run_len) return 0;
    HIPCHK(b_rs.alloc((uint64_t)R * sizeof(uint32_t)));
    HIPCHK(b_rq.alloc((uint64_t)R * sizeof(int16_t)));
    HIPCHK(b_rconf.alloc((uint64_t)R * sizeof(double)));
    HIPCHK(hipMemsetAsync(b_rconf.get(), 0xff, (uint64_t)R * sizeof(double), c->stream));
    hipLaunchKernelGGL(hml_k_post_run_scatter, dim3(n_chunks), dim3(256), 0, c->stream, p.q.as<int16_t>(), p.conf.as<double>(), c->d_starts.get(), M, d_rc, b_rs.as<uint32_t>(),
                       b_rq.as<int16_t>(), b_rconf.as<unsigned long long>());
    KLAUNCH_CHECK();
    std::vector<uint32_t> h_rs(R);
    std::vector<int16_t> h_rq(R);
    HIPCHK(hipMemcpyAsync(h_rs.data(), b_rs.get(), (uint64_t)R * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(h_rq.data(), b_rq.get(), (uint64_t)R * sizeof(int16_t), hipMemcpyDeviceToHost, c->stream));
    if (run_conf) HIPCHK(hipMemcpyAsync(run_conf, b_rconf.get(), (uint64_t)R * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    lengths_of(h_rs.data(), (uint64_t)R, (uint32_t)c->T, run_len);
    if (run_state) std::copy(h_rq.begin(), h_rq.end(), run_state);
    return 0;
}

int hml_posterior_terms(hml_ctx* c, float* e, float* m, double* alpha, double* cval, double* beta) {
    NEED_MODEL();
    const int K = c->K;
    if (e || m) {
        post_tables t;
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
    if (!c->post.computed) return set_err(HML_ERR_ARG, "hml_posterior_info: nothing was computed yet");
    if (chunks) *chunks = c->post.chunks;
    if (L) *L = c->post.used_L;
    if (W) *W = c->post.used_W;
    if (stale_fwd) *stale_fwd = c->post.stale_fwd;
    if (stale_bwd) *stale_bwd = c->post.stale_bwd;
    if (rounds) *rounds = c->post.rounds_run;
    if (serial_chunks) *serial_chunks = c->post.walked;
    return 0;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------- expectation-maximisation (hml_k_em.h)
// The E-step's expected counts behind a smoothing pass, the M-step of hml_em_ref.h on the host, and the fit.  Device memory is
// local to a call, as the smoothing's is.
#include "hml_em_ref.h"
#include "hml_k_em.h"   // (launched from this object alone)

template <int KM>
static void em_launch_norm(hml_ctx* c, const hml_post_args& a, size_t lds, uint32_t B, const double* alpha, const double* beta, double* X, unsigned long long* n_bad) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_k_em_norm<KM>), dim3((B - 1u + 63u) / 64u), dim3(64), lds, c->stream, a, alpha, beta, X, n_bad);
}
#define EM_BY_K(K, fn, ...) do { if ((K) <= 8) fn<8>(__VA_ARGS__); else if ((K) <= 16) fn<16>(__VA_ARGS__); else fn<HML_CAP_K>(__VA_ARGS__); } while (0)

// the E-step: a smoothing pass, then the counts
static int em_estep(hml_ctx* c, hml_em_counts& out) {
    post_tables t;
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
        hml_post_args a;
        a.par = t.par.as<hml_vit_par>(); a.A = t.A.as<double>(); a.pi = t.pi.as<double>();
        a.ia = c->d_ia; a.starts = c->d_starts.get();
        a.L = 0; a.W = 0; a.n_chunks = 0; a.entry = nullptr; a.exitv = nullptr; a.rows = nullptr; a.cval = nullptr; a.ell = nullptr;
        EM_BY_K(K, em_launch_norm, c, a, ((size_t)KK + K) * sizeof(double), B, p.alpha.as<double>(), p.beta.as<double>(), b_X.as<double>(), b_bad.as<unsigned long long>());
        KLAUNCH_CHECK();
    }
    hml_em_args e;
    e.par = t.par.as<hml_vit_par>(); e.A = t.A.as<double>(); e.ia = c->d_ia; e.starts = c->d_starts.get();
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
    out.xi.assign(cols.begin(), cols.begin() + KK);
    if (B == 1u) out.xi.assign((size_t)KK, 0.0);
    out.occ.assign(cols.begin() + KK, cols.begin() + KK + K);
    out.stay.assign(cols.begin() + KK + K, cols.begin() + KK + 2 * K);
    out.sx.resize((size_t)K * D); out.sxx.resize((size_t)K * D);
    for (int j = 0; j < K; ++j)
        for (int d = 0; d < D; ++d) {
            out.sx[j * D + d] = cols[KK + (2 + d) * K + j];
            out.sxx[j * D + d] = cols[KK + (2 + D + d) * K + j];
        }
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
#include <limits>

#include "hml_em_many_ref.h"
#include "hml_k_em_many.h"   // (launched from this object alone)

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

template <int KM, int DIR>
static void em_many_launch_first(hml_ctx* c, const hml_em_many_rec* recs, const em_many_geom& g, uint32_t n, size_t lds) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_k_em_many_first<KM, DIR>), dim3((g.n_chunks + 63u) / 64u, n), dim3(64), lds, c->stream, recs);
}
template <int KM, int DIR>
static void em_many_launch_rerun(hml_ctx* c, const hml_em_many_rec* recs, uint32_t max_heads, uint32_t n, size_t lds) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_k_em_many_rerun<KM, DIR>), dim3((max_heads + 63u) / 64u, n), dim3(64), lds, c->stream, recs);
}
template <int KM, int DIR>
static void em_many_launch_finish(hml_ctx* c, const hml_em_many_rec* recs, uint32_t n, size_t lds) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_k_em_many_finish<KM, DIR>), dim3(1, n), dim3(64), lds, c->stream, recs);
}
template <int KM>
static void em_many_launch_norm(hml_ctx* c, const hml_em_many_rec* recs, const em_many_geom& g, uint32_t n, size_t lds) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_k_em_many_norm<KM>), dim3((g.B - 1u + 63u) / 64u, n), dim3(64), lds, c->stream, recs);
}

// one direction of the smoothing for the first n records: post_direction's rounds, the counts of all members in one copy each
template <int DIR>
static int em_many_direction(hml_ctx* c, const em_many_geom& g, em_many_bufs& b, uint32_t n, em_many_stats& st) {
    const hml_em_many_rec* const recs = b.recs.as<hml_em_many_rec>();
    const size_t lds = ((size_t)g.K * g.K + g.K) * sizeof(double);
    POST_BY_K(g.K, DIR, em_many_launch_first, c, recs, g, n, lds);
    KLAUNCH_CHECK();
    std::vector<uint32_t> h_cnt(2 * (size_t)n);
    bool any = false;
    for (uint32_t round = 0;; ++round) {
        HIPCHK(hipMemsetAsync(b.cnt.get(), 0, h_cnt.size() * sizeof(uint32_t), c->stream));
        hipLaunchKernelGGL(hml_k_em_many_verify, dim3(grid_for(g.n_chunks, 256, 1, 4096), n), dim3(256), 0, c->stream, recs, DIR, g.K);
        KLAUNCH_CHECK();
        HIPCHK(hipMemcpyAsync(h_cnt.data(), b.cnt.get(), h_cnt.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        uint64_t stale = 0;
        uint32_t max_heads = 0;
        for (uint32_t i = 0; i < n; ++i) { stale += h_cnt[2 * i]; max_heads = std::max(max_heads, h_cnt[2 * i + 1]); }
        if (round == 0) st.stale[DIR] += stale;
        any = stale != 0;
        if (!any || round >= c->post.rounds) break;
        POST_BY_K(g.K, DIR, em_many_launch_rerun, c, recs, max_heads, n, lds);
        KLAUNCH_CHECK();
        st.rounds = std::max<uint64_t>(st.rounds, round + 1u);
    }
    if (any) {
        POST_BY_K(g.K, DIR, em_many_launch_finish, c, recs, n, lds);
        KLAUNCH_CHECK();
    }
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
        EM_BY_K(K, em_many_launch_norm, c, recs, g, n, ((size_t)K * K + K) * sizeof(double));
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
    const int K = g.K, D = g.D, KK = K * K;
    out.xi.assign(row, row + KK);
    if (g.B == 1u) out.xi.assign((size_t)KK, 0.0);
    out.occ.assign(row + KK, row + KK + K);
    out.stay.assign(row + KK + K, row + KK + 2 * K);
    out.sx.resize((size_t)K * D); out.sxx.resize((size_t)K * D);
    for (int j = 0; j < K; ++j)
        for (int d = 0; d < D; ++d) {
            out.sx[j * D + d] = row[KK + (2 + d) * K + j];
            out.sxx[j * D + d] = row[KK + (2 + D + d) * K + j];
        }
    const double* const tail = row + g.ncols;
    out.first.assign(tail, tail + K);
    out.loglik = tail[K];
    uint64_t w[HML_EMM_WORDS];
    memcpy(w, tail + K + 1, sizeof w);
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
    hml_model m; if (int r = fetch_model(c, &m)) return r;
    if (int r = post_ready(m)) return r;
    em_many_geom g;
    g.K = c->K; g.D = c->D; g.P = m.P; g.B = m.B;
    const int K = g.K, KK = K * K, P = g.P;
    for (uint64_t r = 0; r < R; ++r) {
        const std::string why = em_many_refusal(P, mean_var + r * 2u * P);
        if (!why.empty()) return set_err(HML_ERR_MODEL, why + " (start " + std::to_string(r) + ")");
    }
    em_params q0;
    em_params_of(m, K, q0);
    g.L = c->post.L ? c->post.L : HML_POST_DEFAULT_L;
    g.W = c->post.W ? c->post.W : HML_POST_DEFAULT_W;
    g.n_chunks = (uint32_t)(((uint64_t)g.B + g.L - 1u) / g.L);
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
            f.par = r.par; f.A = r.A; f.pi = r.pi; f.ia = c->d_ia; f.starts = c->d_starts.get();
            f.L = g.L; f.W = g.W; f.n_chunks = g.n_chunks;
            f.entry = b.entry.as<double>() + i * CK; f.exitv = b.exitv.as<double>() + i * CK;
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
#include "hml_k_pairs.h"   // (launched from this object alone; it brings hml_pairs_ref.h)

struct pairs_result {
    post_result post;   // alpha and beta (c_b, the calls and their confidences are released)
    DevBuf col, p, r;   // [2 K + 1][B] words: the terms, then their inclusive prefix sums; p[B]; r[B][K] for the probe alone
    uint64_t bad = 0;
    uint32_t B = 0;
};

template <int KM>
static void pairs_launch_terms(hml_ctx* c, const hml_post_args& a, size_t lds, uint32_t B, const double* alpha, const double* beta, unsigned long long* col, double* p,
                               double* r, unsigned long long* n_bad) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_k_pair_terms<KM>), dim3((B + 63u) / 64u), dim3(64), lds, c->stream, a, alpha, beta, col, p, r, n_bad);
}

// a smoothing pass, then the terms per block; the prefix sums only if asked (the probe reads the terms themselves)
static int pairs_compute(hml_ctx* c, bool want_r, bool scan, pairs_result& out) {
    post_tables t;
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
    hml_post_args a;
    a.par = t.par.as<hml_vit_par>(); a.A = t.A.as<double>(); a.pi = t.pi.as<double>();
    a.ia = c->d_ia; a.starts = c->d_starts.get();
    a.L = 0; a.W = 0; a.n_chunks = 0; a.entry = nullptr; a.exitv = nullptr; a.rows = nullptr; a.cval = nullptr; a.ell = nullptr;
    EM_BY_K(K, pairs_launch_terms, c, a, ((size_t)K * K + K) * sizeof(double), B, out.post.alpha.as<double>(), out.post.beta.as<double>(), out.col.as<unsigned long long>(),
            out.p.as<double>(), out.r.as<double>(), b_bad.as<unsigned long long>());
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

// Shared by the four kinds of translation unit of libhammlet_hip.so's chain code (hammlet_amd/build.py):
//   hml_capi.hip  - the C ABI (include/hml.h) and everything that does not depend on the number of states K: one object.  It
//                   includes hml_rtk_sweep.hpp, the sweeps of the two paths that take K at run time (the reference-compatible mode,
//                   more than 16 states) behind tables of their own (hml_ktab_compat, hml_ktab_wide): their kernels stay in this object;
//   hml_readout.hip - the C ABI's read-outs of what the recorded sweeps accumulated (marginals, levels, agreement, breaks, bands,
//                   regions, payloads, history): one object;
//   hml_infer.hip - exact inference under the current parameters (Viterbi, smoothing, EM, EM from many starts, the exact breakpoint
//                   and region posteriors): one object, whose kernels (hml_k_viterbi.h, hml_k_posterior.h, hml_k_em.h, hml_k_em_many.h,
//                   hml_k_pairs.h) no other object holds.  The host helpers the two share are hml_readout_shared.hpp's;
//   hml_sweep.hip - the sweep for K states: the kernels templated on K and the host code that launches them, behind a table
//                   of function pointers (hml_ktab): fifteen objects, -DHML_TU_K=2 ... 16, compiled in parallel.
// Every object carries its own code object, and the HIP runtime loads a code object when the first kernel of it is launched:
// a run with K states loads the core's (construction, block scan, marginals) and the one of its K (1-2 MB each), the read-outs'
// and the inference's only if it calls one of them, instead of
// one 19 MB object with every kernel for 2 ... 16 states - 45 ms of a short run's start-up - and the library
// builds in a fifth of the time.  Kernels that are not templates have internal linkage (HML_KERNEL) so that the objects may
// each hold the ones they launch.  (Round 4: this header and the two files were one file sliced by the preprocessor.)
// The core reaches a context's sweep, parameter kernel and buffer allocation through the table hml_set_model chose for it
// (hml_ctx::kt) and never asks which path it is.  What a sweep launches is decided by a pure function per family of paths
// (hml_sweep_plan.h, hml_rtk_plan.h), where the arrays of a carved buffer lie by one layout function per buffer
// (hml_layouts.h); neither header needs HIP, and the CPU tests hold them to their rules.
// Development builds for one K (tools/dev_build.py): every csrc/*.hip with -DHML_ONLY_K=k.
#ifndef HML_CAPI_SHARED_HPP
#define HML_CAPI_SHARED_HPP

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/hml.h"
#include "hml_k_backward.h"
#include "hml_k_blocks.h"
#include "hml_k_blocks_fused.h"
#include "hml_k_blocks_fused_many.h"
#include "hml_k_build.h"
#include "hml_k_forward.h"
#include "hml_k_marginals.h"
#include "hml_k_scan.h"
#include "hml_k_levels.h"
#include "hml_k_breaks.h"
#include "hml_k_bands.h"
#include "hml_k_regions.h"
#include "hml_k_segment.h"
#include "hml_k_trellis.h"
#include "hml_k_trellis_rows.h"
#include "hml_k_compat.h"
#include "hml_k_wide.h"
#include "hml_k_wide_lanes.h"
#include "hml_k_blocks_split_many.h"
#include "hml_k_many.h"
#include "hml_k_params.h"
#include "hml_state.h"
#include "hml_synth_host.hpp"

#include "hml_host_common.hpp"
#include "hml_ctx.hpp"

int hml_set_err(int code, const std::string& msg);   // hml_capi.hip (the thread's last error message)
static int set_err(int code, const std::string& msg) { return hml_set_err(code, msg); }


// What the core calls of a context's path: one table per number of states on the default path (defined at the end of
// hml_sweep.hip), one each for the reference-compatible mode and for more than 16 states (hml_rtk_sweep.hpp).  hml_set_model
// chooses the table and the context keeps it (hml_ctx::kt).
struct hml_ktab {
    int (*sweep)(hml_ctx* c, char method, bool record);
    // (null where chains are never batched: many_eligible refuses them)
    int (*iterate_many)(hml_ctx* const* cs, int n, uint64_t first, uint64_t iterations, uint64_t thinning, uint64_t* done);
    void (*params)(hml_ctx* c, int mode);        // the parameter kernel: 1 = draw from the priors, 2 = Theta's constructor draw
    void (*derive)(hml_ctx* c);                  // what the kernels derive from parameters that were set (hml_set_parameters)
    int (*alloc_sweep)(hml_ctx* c);              // the per-block sweep buffers, sized by the context's block capacity (c->K set)
};
__attribute__((visibility("hidden"))) int hml_alloc_sweep_default(hml_ctx* c);   // hml_capi.hip: ... of the default path, whatever its K

// Live contexts per device.  The fused block kernel hands block offsets from workgroup to workgroup inside one launch
// (a workgroup spins on the words of lower-numbered ones); that is safe while all lower-numbered workgroups are resident
// or finished, which in-order dispatch guarantees for ONE kernel on the GPU.  With two chains sweeping the same GPU at
// once the eight XCDs can fill up with the late workgroups of one launch and the early ones of the other, each waiting
// for workgroups that cannot be dispatched (observed once under the profiler: two launches stalled for 27 s until the
// firmware's time slicing untangled them).  So while more than one context is alive on a device every sweep takes the
// scan + scatter pair, which has no such hand-off.
extern std::atomic<int> hml_live_ctx[64];   // hml_capi.hip
#define g_live_ctx hml_live_ctx
static bool shares_device(const hml_ctx* c) { return c->device < 64 && g_live_ctx[c->device].load() > 1; }
// the plan of the chain's next sweep from the hint as it stands (hml_sweep_plan.h; h_B[1]: a bounded wait of the fused block kernel expired)
static hml_sweep_plan plan_of(const hml_ctx* c, bool mix, bool wait_expired) {
    return hml_plan_sweep(c->knobs, c->T, c->D, mix, c->B_hint, !shares_device(c), wait_expired);
}


// ------------------------------------------------------------------------------------------------
static int ctx_bind(hml_ctx* c) {
    HIPCHK(hipSetDevice(c->device));
    return 0;
}

static hipEvent_t ev_get(hml_ctx* c) {
    if (!c->ev_pool.empty()) { hipEvent_t e = c->ev_pool.back(); c->ev_pool.pop_back(); return e; }
    hipEvent_t e;
    hipEventCreate(&e);
    return e;
}

struct ProfScope {
    hml_ctx* c; const char* name; hipEvent_t a = nullptr, b = nullptr;
    bool on;
    ProfScope(hml_ctx* c_, const char* n, int level = 2) : c(c_), name(n), on(c_->profiling >= level) {
        // level 1 (the bench's timed region): bracket every 32nd launch only - two event records cost ~6 us of
        // stream time, a visible share of an 80 us sweep
        // (a counter per family: the weakly compressed sweep has two level-1 families, block scan and first trellis pass)
        if (on && c->profiling == 1 && (c->prof[name].tick++ & 31u) != 0u) on = false;
        if (on) { a = ev_get(c); b = ev_get(c); hipEventRecord(a, c->stream); }
    }
    ~ProfScope() {
        if (!on) return;
        hipEventRecord(b, c->stream);
        c->prof[name].pending.push_back({a, b});
        if (c->profiling == 1) {
            // an empty bracket right behind: what two event records measure with nothing in between ("event_null")
            hipEvent_t n0 = ev_get(c), n1 = ev_get(c);
            hipEventRecord(n0, c->stream);
            hipEventRecord(n1, c->stream);
            c->prof["event_null"].pending.push_back({n0, n1});
        }
    }
};

// a captured sweep that no longer matches the context's settings or buffers goes (the context's device is current)
static void drop_graph(hml_ctx* c) {
    if (c->graph_exec) { hipGraphExecDestroy(c->graph_exec); c->graph_exec = nullptr; }
}

// the block count the grids of a sweep are sized for: the hint, or a guess while no enumeration has reported yet
static uint32_t grid_hint(const hml_ctx* c) { return c->B_hint ? c->B_hint : (uint32_t)std::min<uint64_t>(c->T, 1u << 20); }
// where the probed emission terms / forward rows go (none unless hml_enable_probes)
static float* eprobe_of(const hml_ctx* c) { return c->probes ? c->d_eprobe.get() : nullptr; }
static float* aprobe_of(const hml_ctx* c) { return c->probes ? c->d_aprobe.get() : nullptr; }

// is the stream being captured into a graph?  (an error of the query: no)
static bool capturing(hipStream_t s) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    return hipStreamIsCapturing(s, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone;
}

static int grid_for(uint64_t items, int per_block, int lo, int hi) {
    uint64_t g = (items + per_block - 1) / per_block;
    if (g < (uint64_t)lo) g = lo;
    if (g > (uint64_t)hi) g = hi;
    return (int)g;
}

static const char* deverr_text(uint32_t code, float v, char* buf, size_t n) {
    switch (code) {
        case HML_DEVERR_IP_NOT_FINITE: snprintf(buf, n, "Result of Normal inner product is not finite!"); break;
        case HML_DEVERR_NEG_BACKWARD: snprintf(buf, n, "Negative backward variable!"); break;
        case HML_DEVERR_NEG_SUMSQ: snprintf(buf, n, "Sum of squares is negative (%s)!", std::to_string(v).c_str()); break;
        case HML_DEVERR_NIG_ALPHA: snprintf(buf, n, "Alpha (%s) must be positive!", std::to_string(v).c_str()); break;
        case HML_DEVERR_NIG_BETA: snprintf(buf, n, "Beta (%s) must be positive!", std::to_string(v).c_str()); break;
        case HML_DEVERR_NIG_NU: snprintf(buf, n, "Nu (%s)must be positive!", std::to_string(v).c_str()); break;
        case HML_DEVERR_NIG_MU0: snprintf(buf, n, "Mu0 (%s)  must be finite!", std::to_string(v).c_str()); break;
        case HML_DEVERR_MEAN_NOT_FINITE: snprintf(buf, n, "Mean (%s) must be set to a finite value!", std::to_string(v).c_str()); break;
        case HML_DEVERR_VAR_NOT_FINITE: snprintf(buf, n, "Variance(%s) must be set to a finite value!", std::to_string(v).c_str()); break;
        case HML_DEVERR_VAR_NOT_POSITIVE: snprintf(buf, n, "Variance (%s) must be positive!", std::to_string(v).c_str()); break;
        case HML_DEVERR_TOO_MANY_RECORDS: snprintf(buf, n, "Too many recorded iterations for the marginal counters!"); break;
        case HML_DEVERR_LAUNCH_GEOMETRY: snprintf(buf, n, "internal error: a one-wavefront kernel was launched with %d threads per workgroup", (int)v); break;
        default: snprintf(buf, n, "device error %u", code);
    }
    return buf;
}

static int fetch_model(hml_ctx* c, hml_model* out) {
    HIPCHK(hipMemcpyAsync(out, c->d_mdl, sizeof(hml_model), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

static int check_device_error(hml_ctx* c) {
    // (the two error words only: the model is 100 KB since its arrays hold HML_CAP_K states)
    struct { uint32_t code; float value; } e;
    static_assert(offsetof(hml_model, err_value) == offsetof(hml_model, err_code) + sizeof(uint32_t), "err_code and err_value are read together");
    HIPCHK(hipMemcpyAsync(&e, &c->d_mdl->err_code, sizeof e, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (e.code != 0) {
        char buf[256];
        return set_err(HML_ERR_MODEL, deverr_text(e.code, e.value, buf, sizeof buf));
    }
    return 0;
}



// ---------------------------------------------------------------------------------------- blocks
// K4: scan (the HBM-bound kernel) + scatter with in-kernel offsets
static void launch_compact_pair(hml_ctx* c, int mode, float thr) {
    // mode 0: model threshold; 1: explicit threshold
    const uint32_t n_groups = (c->n_spans + HML_GROUP_SPANS - 1) / HML_GROUP_SPANS;
    const int scan = hml_plan_scan(c->knobs, c->T, c->B_hint);   // (summary, float stream, or float stream staging flags: hml_sweep_plan.h)
    const bool bits = scan == HML_SCAN_FLAGS;
    {
        ProfScope ps(c, "blocks_compact", 1);
        if (scan == HML_SCAN_SUMMARY) {
            hipLaunchKernelGGL(hml_k_compact_scan_summary, dim3(n_groups), dim3(256), 0, c->stream, c->d_summary, c->d_w,
                               (uint32_t)c->T, c->d_mdl, thr, mode, c->key_base, c->d_stage, c->d_span_count, c->d_coarse1);
        } else if (bits) {
            hipLaunchKernelGGL(hml_k_compact_scan_bits, dim3((c->n_spans + 3) / 4), dim3(256), 0, c->stream, c->d_w, (uint32_t)c->T,
                               c->d_mdl, thr, mode, c->d_stage.as<unsigned long long>(), c->d_span_count);
        } else {
            hipLaunchKernelGGL(hml_k_compact_scan, dim3((c->n_spans + 3) / 4), dim3(256), 0, c->stream, c->d_w, (uint32_t)c->T,
                               c->d_mdl, thr, mode, c->d_stage, c->d_span_count);
        }
    }
    {
        ProfScope ps(c, "blocks_scatter");
        if (scan != HML_SCAN_SUMMARY)
            hipLaunchKernelGGL(hml_k_group_totals, dim3((n_groups + 255) / 256), dim3(256), 0, c->stream, c->d_span_count,
                               c->n_spans, c->d_coarse1);
        if (bits)
            hipLaunchKernelGGL(hml_k_compact_scatter_bits, dim3(n_groups), dim3(256), 0, c->stream, c->d_stage.as<const unsigned long long>(),
                               c->d_span_count, c->d_coarse1, c->n_spans, (uint32_t)c->T, c->d_mdl, c->d_starts, c->d_hB);
        else
        hipLaunchKernelGGL(hml_k_compact_scatter, dim3(n_groups), dim3(256), 0, c->stream, c->d_stage, c->d_span_count,
                           c->d_coarse1, c->n_spans, (uint32_t)c->T, c->d_mdl, c->d_starts, c->d_hB);
    }
}

static int launch_compact(hml_ctx* c, bool use_override, float thr) {
    launch_compact_pair(c, use_override ? 1 : 0, thr);
    KLAUNCH_CHECK();
    {
        ProfScope ps(c, "block_stats");
        const uint32_t hint = grid_hint(c);
        for (int d = 0; d < c->D; ++d)   // the same enumeration for every dimension (dimension-major planes)
            hipLaunchKernelGGL(hml_k_block_stats, dim3(grid_for(hint, 256, 64, 16384)), dim3(256), 0, c->stream,
                               c->d_ia + (uint64_t)d * (c->T + 1), c->d_starts, c->d_mdl, c->d_bstat + (uint64_t)d * c->T);
    }
    KLAUNCH_CHECK();
    return 0;
}

// how sweep_compat and sweep_wide begin: starts, block count, block statistics at the model's threshold
static int launch_blocks_if_needed(hml_ctx* c) {
    if (!c->dynamic && c->blocks_valid) return 0;
    if (int r = launch_compact(c, false, 0.0f)) return r;
    if (!c->dynamic) c->blocks_valid = true;
    return 0;
}

// capacity-limited contexts (hml_ctx.hpp): every enqueued sweep is noted, so that sweeps a halted chain skipped can be run again
static inline bool cap_limited(const hml_ctx* c) { return c->cap != 0 && c->cap < c->T; }
static inline bool chain_halted(const hml_ctx* c) { return cap_limited(c) && ((volatile uint32_t*)c->h_B)[2] != 0u; }
static inline void log_sweep(hml_ctx* c, char method, bool record) {
    c->requested++;
    if (cap_limited(c)) c->sweep_log.push_back((uint8_t)((method == HML_METHOD_MIXTURE ? 1 : 0) | (record ? 2 : 0)));
}
static inline int settle_if_limited(hml_ctx* c) { return cap_limited(c) ? hml_settle(c) : 0; }

// how an entry point of the C ABI begins: a context with a model (with observations), its device current, no halted sweep left behind
#define NEED_MODEL() if (!c || !c->model_set) return set_err(HML_ERR_ARG, "model not set"); if (int r_ = ctx_bind(c)) return r_; if (int r_ = settle_if_limited(c)) return r_
#define NEED_LOADED() if (!c || !c->loaded) return set_err(HML_ERR_ARG, "no observations loaded"); if (int r_ = ctx_bind(c)) return r_; if (int r_ = settle_if_limited(c)) return r_

static void refresh_hint(hml_ctx* c) {
    const uint32_t b = *(volatile uint32_t*)c->h_B;
    if (b) c->B_hint = b + b / 4 + 1024;
}


static int ensure_marginal_buffers(hml_ctx* c) {
    if (c->d_diff) return 0;
    const uint64_t n = (uint64_t)c->K * (c->T + 1);
    const uint64_t words = (c->T + 1 + 31) / 32 + 1;
    HIPCHK(c->d_boundary.alloc(words));
    HIPCHK(c->d_diff.alloc(n));   // (last: it is what tells that both are there)
    HIPCHK(hipMemsetAsync(c->d_diff, 0, n * sizeof(int32_t), c->stream));
    HIPCHK(hipMemsetAsync(c->d_boundary, 0, words * sizeof(uint32_t), c->stream));
    return 0;
}

// recorded sweeps cannot go into marginals that are a pooled payload (`whose`: "this context" / "a context")
static int pooled_refusal(const hml_ctx* c, bool record, const char* whose) {
    if (!(record && c->rec_marginals && c->pooled)) return 0;
    return set_err(HML_ERR_ARG, std::string("the marginals of ") + whose + " are pooled (common labels, several chains): further sweeps cannot be recorded into them");
}
// the state marginals of a recorded sweep (bracket: as profile family "marginals" - the default path's sweeps)
static int launch_marginals(hml_ctx* c, hipStream_t s, uint32_t hint, bool bracket) {
    if (!c->rec_marginals) return 0;
    if (int r = pooled_refusal(c, true, "this context")) return r;
    if (int r = ensure_marginal_buffers(c)) return r;
    ProfScope ps(c, "marginals", bracket ? 2 : 1 << 30);
    hipLaunchKernelGGL(hml_k_record, dim3(grid_for(hint, 256, 64, 16384)), dim3(256), 0, s, c->d_q, c->d_starts, c->d_mdl, c->d_diff, c->d_boundary);
    return 0;
}

// ---- the per-position recordings beside the marginals (hml_recorder, hml_ctx.hpp): what differs between the three ----
struct hml_recorder_kind {
    const char* family;   // profile family of its record kernel
    size_t elem;          // bytes of an accumulator cell
    size_t counter;       // offset in hml_model of its count of recorded sweeps
    const char* none;     // "nothing was recorded" (%s: "this" / "the source")
    const char* noun;     // what the merge messages call it
    const char* file;     // ... and its output file
};
static const hml_recorder_kind hml_recorder_kinds[HML_REC_KINDS] = {
    {"levels", sizeof(double), offsetof(hml_model, n_levels_recorded),
     "no emission levels were recorded by %s context: enable them with hml_set_level_recording (or HML_LEVELS=1) before the recorded sweeps", "emission levels", "levels"},
    {"breaks", sizeof(uint32_t), offsetof(hml_model, n_breaks_recorded),
     "no breakpoints were recorded by %s context: enable them with hml_set_break_recording (or HML_BREAKS=1) before the recorded sweeps", "breakpoints", "breakpoints"},
    {"bands", sizeof(int32_t), offsetof(hml_model, n_bands_recorded),
     "no level bands were recorded by %s context: give the edges with hml_set_level_bands (or HML_BANDS=e0,e1,...) before the recorded sweeps", "level bands", "bands"},
};
static int recorder_rows(const hml_ctx* c, int kind) {
    return kind == HML_REC_LEVELS ? 2 * c->D : kind == HML_REC_BREAKS ? 1 : c->D * (c->n_band_edges + 1);
}
static unsigned long long* recorder_counter(const hml_ctx* c, int kind) {
    return (unsigned long long*)(c->d_mdl.as<char>() + hml_recorder_kinds[kind].counter);
}
static int recorder_none(int kind, const char* whose) {
    char buf[256];
    snprintf(buf, sizeof buf, hml_recorder_kinds[kind].none, whose);
    return set_err(HML_ERR_ARG, buf);
}

// a recording's accumulators - rows (T + 1) cells and (T + 32) / 32 words of bitmap - on first use.  Zeroed before this
// returns: chains batched by hml_iterate_many run on their group's stream, not on their own.
static int ensure_recorder_buffers(hml_ctx* c, int kind) {
    hml_recorder& r = c->rec[kind];
    if (r.d_acc) return 0;
    if (kind == HML_REC_BANDS && (c->n_band_edges < 1 || recorder_rows(c, kind) > HML_CAP_K))
        return set_err(HML_ERR_ARG, "level bands: the data dimensions times (edges + 1) must be between 2 and 64 columns");
    const uint64_t bytes = (uint64_t)recorder_rows(c, kind) * (c->T + 1) * hml_recorder_kinds[kind].elem;
    const uint64_t words = (c->T + 32) / 32;
    HIPCHK(r.d_boundary.alloc(words));
    HIPCHK(r.d_acc.alloc(bytes));   // (last: it is what tells that both are there)
    HIPCHK(hipMemsetAsync(r.d_acc.get(), 0, bytes, c->stream));
    HIPCHK(hipMemsetAsync(r.d_boundary, 0, words * sizeof(uint32_t), c->stream));
    if (!capturing(c->stream)) HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}
static int ensure_region_buffers(hml_ctx* c);   // (below)
// ... of every recording that is on
static int ensure_recorders(hml_ctx* c) {
    for (int kind = 0; kind < HML_REC_KINDS; ++kind)
        if (c->rec[kind].on) { if (int r = ensure_recorder_buffers(c, kind)) return r; }
    if (c->rg.on) { if (int r = ensure_region_buffers(c)) return r; }
    return 0;
}

static hml_band_edges band_edges_of(const hml_ctx* c) {
    hml_band_edges ed;
    memset(&ed, 0, sizeof ed);
    ed.n = c->n_band_edges;
    for (int j = 0; j < c->n_band_edges; ++j) ed.e[j] = c->band_edges[j];
    return ed;
}
static bool same_band_edges(const hml_ctx* a, int n, const float* edges) {
    return a->n_band_edges == n && memcmp(a->band_edges, edges, (size_t)n * sizeof(float)) == 0;   // (bit for bit)
}

// the record kernel of one recording, on stream `s`
static void launch_record_kernel(hml_ctx* c, int kind, hipStream_t s, dim3 grid) {
    const hml_recorder& r = c->rec[kind];
    if (kind == HML_REC_LEVELS)
        hipLaunchKernelGGL(hml_k_levels_record, grid, dim3(256), 0, s, c->d_q, c->d_starts, c->d_mdl, r.acc<double>(), r.d_boundary);
    else if (kind == HML_REC_BREAKS)
        hipLaunchKernelGGL(hml_k_breaks_record, grid, dim3(256), 0, s, c->d_q, c->d_starts, c->d_mdl, r.acc<uint32_t>(), r.d_boundary);
    else
        hipLaunchKernelGGL(hml_k_bands_record, grid, dim3(256), 0, s, c->d_q, c->d_starts, c->d_mdl, band_edges_of(c), r.acc<int32_t>(), r.d_boundary);
}

// ---- the joint posteriors over caller-given regions (hml_regions, hml_ctx.hpp; hml_k_regions.h) ----
static const char* const hml_regions_none = "no regions were recorded by %s context: give them with hml_set_regions before the recorded sweeps";
static int regions_none(const char* whose) {
    char buf[256];
    snprintf(buf, sizeof buf, hml_regions_none, whose);
    return set_err(HML_ERR_ARG, buf);
}
static int regions_columns(const hml_ctx* c) { return c->rg.n_edges > 0 ? c->D * (c->rg.n_edges + 1) : 0; }
static hml_band_edges region_edges_of(const hml_ctx* c) {
    hml_band_edges ed;
    memset(&ed, 0, sizeof ed);
    ed.n = c->rg.n_edges;
    for (int j = 0; j < c->rg.n_edges; ++j) ed.e[j] = c->rg.edges[j];
    return ed;
}
static bool same_regions(const hml_ctx* c, uint64_t n, const uint32_t* start, const uint32_t* end, int n_edges, const float* edges) {
    const hml_regions& g = c->rg;
    return g.start.size() == n && g.n_edges == n_edges && memcmp(g.start.data(), start, n * sizeof(uint32_t)) == 0 &&
           memcmp(g.end.data(), end, n * sizeof(uint32_t)) == 0 && (n_edges == 0 || memcmp(g.edges, edges, (size_t)n_edges * sizeof(float)) == 0);   // (bit for bit)
}
// words of 8 bytes per region: whole, breaks_sum, breaks_sq, D level sums, D sums of squares, the band columns
static uint64_t regions_acc_words(const hml_ctx* c) { return 3u + 2u * (uint64_t)c->D + (uint64_t)regions_columns(c); }
static hml_regions_acc regions_acc_views(const hml_ctx* c) {
    const uint64_t n = c->rg.start.size();
    hml_regions_acc a;
    unsigned long long* w = c->rg.d_acc.as<unsigned long long>();
    a.whole = w; a.breaks_sum = w + n; a.breaks_sq = w + 2 * n;
    a.level_sum = (double*)(w + 3 * n);
    a.level_sq = a.level_sum + (uint64_t)c->D * n;
    a.inband = w + (3u + 2u * (uint64_t)c->D) * n;
    return a;
}
// (one entry per chunk of HML_RG_CHUNK blocks; at most T blocks, whatever the block capacity)
static uint32_t regions_chunk_stride(const hml_ctx* c) { return (uint32_t)((c->T + HML_RG_CHUNK - 1u) / HML_RG_CHUNK); }
static hml_regions_chunks regions_chunk_views(const hml_ctx* c) {
    hml_regions_chunks ch;
    ch.stride = regions_chunk_stride(c);
    ch.lev = c->rg.d_chunks.as<double>();
    ch.cnt = (uint32_t*)(ch.lev + (uint64_t)c->D * ch.stride);
    return ch;
}
static int regions_fault(const hml_ctx* c) {   // what only the loaded trace and the model can tell
    const hml_regions& g = c->rg;
    for (size_t r = 0; r < g.start.size(); ++r)
        if (!(g.start[r] < g.end[r] && (uint64_t)g.end[r] <= c->T)) {
            char buf[200];
            snprintf(buf, sizeof buf, "regions: region %llu, [%u, %u), does not lie inside the %llu positions of the trace", (unsigned long long)r, g.start[r], g.end[r],
                     (unsigned long long)c->T);
            return set_err(HML_ERR_ARG, buf);
        }
    if ((uint64_t)c->D * (uint64_t)(g.n_edges + 1) > HML_CAP_K) return set_err(HML_ERR_ARG, "regions: the data dimensions times (edges + 1) exceed 64 columns");
    return 0;
}
// hml_readout.hip: the regions' buffers on first use, and the three launches of a recorded sweep's regions.  Defined in ONE
// object, so that the code objects of the sweeps and of the core hold the kernels they held before.
// (internal to the library: not part of the C ABI, not exported)
__attribute__((visibility("hidden"))) int hml_regions_ensure(hml_ctx* c);
__attribute__((visibility("hidden"))) void hml_regions_launch(hml_ctx* c, hipStream_t s, uint32_t hint, bool bracket);
static int ensure_region_buffers(hml_ctx* c) { return hml_regions_ensure(c); }
static void launch_region_kernels(hml_ctx* c, hipStream_t s, uint32_t hint, bool bracket) { hml_regions_launch(c, s, hint, bracket); }

// ---- the chain's history (hml_history, hml_ctx.hpp; hml_k_history.h) ----
// hml_readout.hip, in that ONE object like the regions: room for the rows of `iterations` further sweeps, made on the host
// before anything is enqueued (a larger buffer drops the captured graph), and the one launch behind a sweep's parameter
// update, on stream `s`.
__attribute__((visibility("hidden"))) int hml_history_ensure(hml_ctx* c, uint64_t iterations);
__attribute__((visibility("hidden"))) void hml_history_launch(hml_ctx* c, hipStream_t s, char method);
static inline bool history_due(const hml_ctx* c) { return c->hist.on && c->hist.d_buf; }
// ... behind the update and the recorders of a sweep on the context's own stream; nothing without a history
static inline void launch_history(hml_ctx* c, char method) {
    if (!history_due(c)) return;
    ProfScope ps(c, "history");
    hml_history_launch(c, c->stream, method);
}

// the record kernels of a recorded sweep, on stream `s`, BEHIND the sweep's parameter update: the level (and its band) is mu
// under the theta that hml_get_theta returns inside the sweep's record callback; the breakpoint kernel reads the sweep's
// states and block starts only
static int launch_recorders(hml_ctx* c, hipStream_t s, uint32_t hint) {
    for (int kind = 0; kind < HML_REC_KINDS; ++kind) {
        if (!c->rec[kind].on) continue;
        if (int r = ensure_recorder_buffers(c, kind)) return r;
        ProfScope ps(c, hml_recorder_kinds[kind].family);
        launch_record_kernel(c, kind, s, dim3(grid_for(hint, 256, 64, 16384)));
    }
    if (c->rg.on) {
        if (int r = ensure_region_buffers(c)) return r;
        ProfScope ps(c, "regions");
        launch_region_kernels(c, s, hint, /*bracket*/ true);
    }
    return 0;
}


// ---- chunk length of the fused trellis path (hml_ctx.hpp: tre_autotune)
#define HML_TRE_TUNE_AFTER 48u   // sweeps before the measurement: the filter's warm-up length has settled by then
// Candidates.  The wavefronts of the first pass (64 chunks each) all do the same work and stay resident from launch to
// exit, so the pass takes a whole number of ROUNDS over the machine's wavefront slots: the chunk lengths worth measuring
// are those that fill 1, 2, 3 ... rounds almost completely (longer chunks = a smaller warm-up share, but longer refits of
// the chunks that fail verification).  hml_k_trellis_tile (HML_TRELLIS_ROWS=0) keeps round 2's list.
static uint32_t tre_default_L_old(uint32_t hint) { return hint >= (1u << 26) ? 128u : hint >= (1u << 24) ? 64u : (uint32_t)HML_TRE_MIN_L; }
static int tre_candidates(const hml_ctx* c, uint32_t hint, uint32_t* out) {
    int n = 0;
    if (!c->knobs.tre_rows || c->tre_slots <= 0) {
        const uint32_t L0 = tre_default_L_old(hint);
        for (uint32_t q = 4; q <= 8; ++q) {   // L0 * {1, 1.25, 1.5, 1.75, 2}, multiples of 32
            const uint32_t l = L0 * q / 4u;
            if (l % 32u == 0u && l <= 256u) out[n++] = l;
        }
        return n;
    }
    // (the hint is the last sweep's block count with a quarter of headroom - what the grids are sized for; the rounds are
    // counted over the blocks themselves)
    const uint32_t blocks = hint > 1024u ? (uint32_t)(((uint64_t)hint - 1024u) * 4u / 5u) : hint;
    for (uint32_t rounds = 1; rounds <= 8u && n < 6; ++rounds) {
        const double waves = 0.985 * (double)c->tre_slots * rounds;              // (a little air: one wavefront too many costs a round)
        uint32_t l = (uint32_t)((double)blocks / (64.0 * waves)) + 1u;
        l = (l + 31u) / 32u * 32u;
        if (l < (uint32_t)HML_TRE_MIN_L) l = HML_TRE_MIN_L;
        // (without checkpoints a refit walks its whole chunk: beyond 512 rows that costs more than the warm-up saves)
        if (l > (c->tre_ckpt ? (uint32_t)HML_TRE_MAX_L : 512u)) continue;
        bool seen = false;
        for (int i = 0; i < n; ++i) seen = seen || out[i] == l;
        if (!seen) out[n++] = l;
        if (l == (uint32_t)HML_TRE_MIN_L) break;
    }
    if (n == 0) out[n++] = 512u;
    return n;
}
static uint32_t tre_default_L(const hml_ctx* c, uint32_t hint) {   // until the measurement: two rounds where there are blocks for them
    if (!c->knobs.tre_rows || c->tre_slots <= 0) return tre_default_L_old(hint);
    uint32_t cand[8];
    const int n = tre_candidates(c, hint, cand);
    return cand[n > 1 ? 1 : 0];
}
static bool tre_tuned_for(const hml_ctx* c, uint32_t hint) {
    return c->tre_tuned_L && hint <= c->tre_tuned_hint + c->tre_tuned_hint / 8u && hint + hint / 8u >= c->tre_tuned_hint;
}
// does the next fused-trellis sweep measure a candidate?  (it then runs outside any graph and waits for its own events)
static bool tre_wants_measurement(const hml_ctx* c, uint32_t hint) {
    return !c->tre_L && c->tre_autotune && !tre_tuned_for(c, hint) && c->tre_dense_sweeps >= HML_TRE_TUNE_AFTER;
}
// the chunk length of the next sweep; *measure: bracket the trellis kernels with events and report (tre_tune_report)
static uint32_t tre_pick_L(hml_ctx* c, uint32_t hint, bool capturing, bool* measure) {
    *measure = false;
    if (c->tre_L) return c->tre_L;
    if (tre_tuned_for(c, hint)) return c->tre_tuned_L;
    if (capturing || !tre_wants_measurement(c, hint)) return c->tre_tuned_L ? c->tre_tuned_L : tre_default_L(c, hint);
    if (c->tre_tune_step < 0) {
        // a measurement starts: its candidates are fixed now (the block count drifts over the 2 n measuring sweeps, and the
        // list with it: timings of different lengths would mix, and the winner might never have been measured)
        c->tre_cand_n = tre_candidates(c, hint, c->tre_cand);
        if (c->tre_cand_n < 2) { c->tre_tuned_L = c->tre_cand[0]; c->tre_tuned_hint = hint; return c->tre_cand[0]; }
        c->tre_tune_step = 0;
        for (float& v : c->tre_tune_ms) v = 3.4e38f;
    }
    *measure = true;
    return c->tre_cand[c->tre_tune_step % c->tre_cand_n];
}
static void tre_tune_report(hml_ctx* c, uint32_t hint, float ms) {
    const uint32_t* const cand = c->tre_cand;
    const int n = c->tre_cand_n;
    const int i = c->tre_tune_step % n;
    c->tre_tune_ms[i] = std::min(c->tre_tune_ms[i], ms);
    if (++c->tre_tune_step < 2 * n) return;
    int best = 0;
    for (int k = 1; k < n; ++k) if (c->tre_tune_ms[k] < c->tre_tune_ms[best]) best = k;
    c->tre_tuned_L = cand[best];
    c->tre_tuned_hint = hint;
    c->tre_tune_step = -1;
    if (getenv("HML_TRELLIS_TUNE_DEBUG")) {
        fprintf(stderr, "[trellis tune] %u blocks:", hint);
        for (int k = 0; k < n; ++k) fprintf(stderr, " L=%u %.3f ms", cand[k], c->tre_tune_ms[k]);
        fprintf(stderr, " -> L=%u\n", cand[best]);
    }
}


// ---- several chains of one device in one set of launches (hml_k_many.h) ----
static bool many_eligible(hml_ctx* const* cs, int n, char method) {
    if (n < 2 || n > 64 || method != HML_METHOD_FB) return false;
    const hml_ctx* a = cs[0];
    for (int i = 0; i < n; ++i) {
        const hml_ctx* c = cs[i];
        if (!c->model_set || c->device != a->device || c->K != a->K || c->T != a->T || c->D != 1 || c->compat || c->wide || !c->dynamic || !c->knobs.use_keys ||
            c->probes || c->profiling || c->knobs.geo[HML_GEO_SPARSE].L != a->knobs.geo[HML_GEO_SPARSE].L ||
            c->knobs.geo[HML_GEO_MANY].L != a->knobs.geo[HML_GEO_MANY].L || c->knobs.late_rescale != a->knobs.late_rescale || c->n_spans != a->n_spans)
            return false;
        for (int j = 0; j < i; ++j) if (cs[j] == c) return false;
    }
    return true;
}
// weakly compressed sweeps (many blocks, or the float stream: hml_sweep_plan.h) keep their own kernels: not batched
static bool many_sparse(hml_ctx* c) {
    refresh_hint(c);
    return !hml_plan_many_blocks(c->knobs, c->B_hint) && !hml_plan_float_stream(c->knobs, c->T, c->B_hint);
}


#endif

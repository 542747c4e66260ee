// The sweeps of the two paths that take the number of states at run time - the reference-compatible mode (hml_k_compat.h) and
// the path for more than 16 states (hml_k_wide.h, hml_k_wide_lanes.h): their buffers, their stages, and the tables
// (hml_ktab_compat, hml_ktab_wide) through which the core reaches them like the sweep of K states.  What a sweep launches is
// hml_plan_rtk's decision (hml_rtk_plan.h), where its carved buffers' arrays lie is hml_layouts.h's: both are tested on the
// CPU.  Included by hml_capi.hip alone: the kernels stay in the core's code object.
#ifndef HML_RTK_SWEEP_HPP
#define HML_RTK_SWEEP_HPP

#include "hml_capi_shared.hpp"

static int rtk_mode(const hml_ctx* c) { return c->wide ? HML_RTK_WIDE : HML_RTK_COMPAT; }
static hml_wl_geometry wl_geometry_of(const hml_ctx* c) { return hml_plan_wl_geometry(c->rtk, c->K); }
// the arrays of d_cchunk, with the plan's warm-up
static hml_compat_chunks chunk_views(const hml_ctx* c, const hml_rtk_plan& p) {
    hml_compat_chunks ch = hml_layout_cchunk(c->d_cchunk.get(), rtk_mode(c), wl_geometry_of(c), c->cap, c->K).ch;
    ch.W = p.W;
    return ch;
}

// The per-block sweep buffers of the reference-compatible mode, sized by the context's block capacity (c->K set): plain emission
// terms [b][s], a plain (B + 1) x K trellis, the states.
static int alloc_sweep_compat(hml_ctx* c) {
    const int K = c->K;
    const uint64_t cap = c->cap;
    HIPCHK(c->d_em.alloc(cap * K));
    HIPCHK(c->d_gsc.alloc(cap * K));
    HIPCHK(c->d_crows.alloc((cap + 1) * K));
    // chunks of the filter and of the backward draws, the engine's outputs of a sweep (two per block), the count pass's lists by state
    HIPCHK(c->d_cchunk.alloc(hml_layout_cchunk(nullptr, HML_RTK_COMPAT, wl_geometry_of(c), cap, K).bytes));
    HIPCHK(c->d_cdraws.alloc(2 * cap));
    HIPCHK(c->d_clists.alloc(hml_layout_clists(nullptr, cap, K).bytes));
    HIPCHK(c->d_q.alloc(cap));
    return 0;
}

// ... of more than 16 states: [b][s] arrays or chunk-transposed ones, the default path's count tree
static int alloc_sweep_wide(hml_ctx* c) {
    const int K = c->K;
    const uint64_t cap = c->cap;
    const hml_wl_geometry g = wl_geometry_of(c);
    const uint64_t plane = hml_wl_plane_floats(g, cap, K);
    HIPCHK(c->d_em.alloc(plane));
    HIPCHK(c->d_gsc.alloc(plane));
    HIPCHK(c->d_crows.alloc(plane));
    const hml_cchunk_layout cl = hml_layout_cchunk(nullptr, HML_RTK_WIDE, g, cap, K);
    HIPCHK(c->d_cchunk.alloc(cl.bytes));
    HIPCHK(hipMemsetAsync(c->d_cchunk.as<char>() + (cl.bytes - cl.tot_bytes), 0, cl.tot_bytes, c->stream));   // (counters and bit maps of wrong chunks)
    HIPCHK(c->d_wA.DevBuf::alloc(hml_layout_wa(nullptr).bytes));
    HIPCHK(c->d_cdraws.alloc(2 * (cap + 1)));
    HIPCHK(c->d_q.alloc(cap));
    const uint64_t n_partial = (uint64_t)HML_REDUCE_GROUPS * K * 2;
    HIPCHK(c->d_partial.alloc(n_partial));
    HIPCHK(hipMemsetAsync(c->d_partial, 0, n_partial * sizeof(double), c->stream));
    HIPCHK(c->d_wacc.alloc(sizeof(hml_wide_acc)));
    HIPCHK(hipMemsetAsync(c->d_wacc.get(), 0, sizeof(hml_wide_acc), c->stream));
    return 0;
}

// filter and backward draws in C chunks with a wavefront each (hml_k_compat.h): the chunks' entry rows against the exit rows
// before them by as many threads as there are elements, then one wavefront that runs the rare wrong chunk again; the same for
// the backward draws.  KC / PAD: the number of states at compile time, or (PAD) an upper bound of the model's.
template <int KC, class M, bool PAD>
static void launch_chunked_fb(hml_ctx* c, hipStream_t s, uint32_t C, const hml_compat_chunks& ch, float* aprobe) {
    {
        ProfScope ps(c, "forward");
        hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_k_compat_forward<KC, M, PAD>), dim3(C), dim3(64), 0, s, c->d_mdl, c->d_em, c->d_gsc, c->d_crows, aprobe, ch);
        if (C > 1u) hipLaunchKernelGGL(hml_k_compat_forward_verify, dim3(grid_for((uint64_t)C * c->K, 256, 1, 4096)), dim3(256), 0, s, c->d_mdl, ch, C);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_k_compat_forward_check<KC, PAD>), dim3(1), dim3(256), 0, s, c->d_mdl, c->d_em, c->d_gsc, c->d_crows, ch, C);
    }
    {
        ProfScope ps(c, "backward_maps");
        hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_k_compat_backward<KC, PAD>), dim3(C), dim3(64), 0, s, c->d_mdl, c->d_crows, c->d_cdraws, c->d_q, ch);
        if (C > 1u) hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_k_compat_backward_check<KC, PAD>), dim3(1), dim3(256), 0, s, c->d_mdl, c->d_crows, c->d_cdraws, c->d_q, ch, C);
    }
}

// ... with a chunk a lane, 64 chunks to a wavefront (hml_k_wide_lanes.h).  KC: the model's number of states rounded up to a multiple of four.
template <int KC>
static void launch_wl_fb(hml_ctx* c, hipStream_t s, const hml_rtk_plan& p, const hml_compat_chunks& ch) {
    constexpr int KS = (KC <= 32) ? 32 : 64;
    const int tiles = grid_for(p.room, (int)std::min<uint64_t>(64 * (uint64_t)p.wl.min_L, 1u << 30), 1, HML_WL_MAX_CHUNKS / 64);
    {
        ProfScope ps(c, "forward");
        hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_k_wl_forward<KC>), dim3(tiles), dim3(64), 0, s, c->d_mdl, c->d_wA, c->d_em, c->d_gsc, c->d_crows, ch, 0);
        hipLaunchKernelGGL(hml_k_wl_forward_verify, dim3(grid_for(p.room / 16 * c->K, 256, 1, 4096)), dim3(256), 0, s, c->d_mdl, ch, 0);
        // many wrong chunks: the filter once more with a longer warm-up (the three launches return at once otherwise)
        hipLaunchKernelGGL(hml_k_wl_retry_decide, dim3(1), dim3(256), 0, s, c->d_mdl, ch);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_k_wl_forward<KC>), dim3(tiles), dim3(64), 0, s, c->d_mdl, c->d_wA, c->d_em, c->d_gsc, c->d_crows, ch, 1);
        hipLaunchKernelGGL(hml_k_wl_forward_verify, dim3(grid_for(p.room / 16 * c->K, 256, 1, 4096)), dim3(256), 0, s, c->d_mdl, ch, 1);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_k_wl_forward_check<KS>), dim3(1), dim3(256), 0, s, c->d_mdl, c->d_em, c->d_gsc, c->d_crows, ch);
    }
    {
        ProfScope ps(c, "backward_maps");
        hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_k_wl_backward<KC>), dim3(tiles), dim3(64), 0, s, c->d_mdl, c->d_crows, c->d_q, ch);
        hipLaunchKernelGGL(hml_k_wl_backward_verify, dim3(grid_for(p.room / 16, 256, 1, 256)), dim3(256), 0, s, c->d_mdl, ch);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_k_wl_backward_check<KS>), dim3(1), dim3(256), 0, s, c->d_mdl, c->d_crows, c->d_q, ch);
    }
}

// how both sweeps begin: starts, block count and block statistics by the default path's kernels, then the plan from the first read of the hint
static int rtk_begin(hml_ctx* c, char method, uint32_t* hint, hml_rtk_plan* p) {
    if (int r = launch_blocks_if_needed(c)) return r;
    refresh_hint(c);
    *hint = grid_hint(c);
    *p = hml_plan_rtk(c->rtk, rtk_mode(c), c->K, c->D, c->T, method == HML_METHOD_MIXTURE, c->probes, *hint);
    return 0;
}

// A sweep of the reference-compatible mode (hml_k_compat.h): the order-dependent part in the reference's order (the number of
// states is a run-time value there), the marginals by hml_k_record.
static int sweep_compat(hml_ctx* c, char method, bool record) {
    hipStream_t s = c->stream;
    uint32_t hint; hml_rtk_plan p;
    if (int r = rtk_begin(c, method, &hint, &p)) return r;
    const int mix = p.mix ? 1 : 0;
    hml_mt_state* const mt = c->d_mt.as<hml_mt_state>();
    hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_k_compat_emission<hml_glibc_exp>), dim3(grid_for(hint, 256, 64, 16384)), dim3(256), 0, s, c->d_mdl, c->d_starts, c->d_bstat, c->d_em, c->d_gsc, mix,
                       eprobe_of(c));
    if (mix) hipLaunchKernelGGL(hml_k_compat_mixture, dim3(1), dim3(64), 0, s, c->d_mdl, mt, c->d_em, c->d_q);
    else {
        // filter and backward draws in chunks with a wavefront each, then one wavefront that checks the chunks in order
        float* const aprobe = aprobe_of(c);
        const hml_compat_chunks ch = chunk_views(c, p);
        hipLaunchKernelGGL(hml_k_compat_draws, dim3(1), dim3(256), 0, s, c->d_mdl, mt, c->d_cdraws, 2u);
#define HML_COMPAT_FB(KC) case KC: launch_chunked_fb<KC, hml_glibc_exp, false>(c, s, p.C, ch, aprobe); break;
        switch (p.pad ? -p.KC : p.KC) {
            HML_COMPAT_FB(2) HML_COMPAT_FB(3) HML_COMPAT_FB(4) HML_COMPAT_FB(5) HML_COMPAT_FB(6) HML_COMPAT_FB(7) HML_COMPAT_FB(8) HML_COMPAT_FB(9)
            HML_COMPAT_FB(10) HML_COMPAT_FB(11) HML_COMPAT_FB(12) HML_COMPAT_FB(13) HML_COMPAT_FB(14) HML_COMPAT_FB(15) HML_COMPAT_FB(16)
            case -32: launch_chunked_fb<32, hml_glibc_exp, true>(c, s, p.C, ch, aprobe); break;
            case -64: launch_chunked_fb<64, hml_glibc_exp, true>(c, s, p.C, ch, aprobe); break;
            default: return set_err(HML_ERR_HIP, "internal error: a model of this many states in the reference-compatible mode");
        }
#undef HML_COMPAT_FB
    }
    // the count pass: by state (partition, then one wavefront over all lists) for long univariate sweeps, in block order otherwise
    const hml_compat_lists pl = hml_layout_clists(c->d_clists.get(), c->cap, c->K).pl;
    if (p.by_state) {
        const unsigned tiles_now = (unsigned)(((uint64_t)hint + hint / 8 + HML_COMPAT_PART_TILE) / HML_COMPAT_PART_TILE);   // (kernels find B themselves; tiles beyond it return)
        const unsigned tg = std::min<uint64_t>(std::max(1u, tiles_now), hml_compat_tiles(c->cap));
        hipLaunchKernelGGL(hml_k_compat_part_count, dim3(tg), dim3(256), 0, s, c->d_mdl, c->d_q, pl);
        hipLaunchKernelGGL(hml_k_compat_part_scan, dim3(1), dim3(64), 0, s, c->d_mdl, pl);
        hipLaunchKernelGGL(hml_k_compat_part_scatter, dim3(tg), dim3(256), 0, s, c->d_mdl, c->d_q, c->d_starts, c->d_bstat, pl);
    }
    hipLaunchKernelGGL(hml_k_compat_update, dim3(1), dim3(p.by_state ? 256 : 64), 0, s, c->d_mdl, mt, c->d_starts, c->d_bstat, c->d_q, mix, pl, p.by_state ? 1 : 0);
    if (record) { if (int r = launch_marginals(c, s, hint, /*bracket*/ false)) return r; }
    if (record) { if (int r = launch_recorders(c, s, hint)) return r; }   // (hml_k_compat_update above is this sweep's parameter update)
    launch_history(c, method);   // (the sweep's row, where the chain keeps a history: hml_k_history.h)
    KLAUNCH_CHECK();
    return 0;
}

// A sweep of a model with more than 16 states (hml_k_wide.h): emission terms / filter / backward draws by the chunk-a-lane kernels
// or the lane-per-state kernels of hml_k_compat.h in this path's arithmetic, the uniforms of the draws from their Philox addresses
// ahead of them, the default path's count tree, hml_k_wide_params.
static int sweep_wide(hml_ctx* c, char method, bool record) {
    hipStream_t s = c->stream;
    uint32_t hint; hml_rtk_plan p;
    if (int r = rtk_begin(c, method, &hint, &p)) return r;
    const int mix = p.mix ? 1 : 0;
    const hml_compat_chunks ch = chunk_views(c, p);
    if (p.form == HML_RTK_LANES) {
        const hml_wa_layout wa = hml_layout_wa(c->d_wA.get());
        hipLaunchKernelGGL(hml_k_wl_prepare, dim3(1), dim3(256), 0, s, c->d_mdl, wa.A, c->rtk.wide_lshift, p.wl.max_chunks);
        hipLaunchKernelGGL(hml_k_wl_gtable, dim3(grid_for((uint64_t)c->K * HML_WL_GTAB, 256, 1, 512)), dim3(256), 0, s, c->d_mdl, wa.gtab);
        {
            ProfScope ps(c, "stats_emission");
            // (a wavefront: 64 chunks x HML_WL_EMIT_ROWS rows)
            hipLaunchKernelGGL(hml_k_wl_emission, dim3(grid_for(p.room, 64 * HML_WL_EMIT_ROWS * 4, 1, 32768)), dim3(256), 0, s, c->d_mdl, c->d_starts, c->d_bstat, c->d_em, c->d_gsc, wa.gtab);
        }
#define HML_WL_FB(KC) case KC: launch_wl_fb<KC>(c, s, p, ch); break;
        switch (p.KC) {
            HML_WL_FB(4) HML_WL_FB(8) HML_WL_FB(12) HML_WL_FB(16)   // (HML_WIDE=1: this path for any model - tests)
            HML_WL_FB(20) HML_WL_FB(24) HML_WL_FB(28) HML_WL_FB(32) HML_WL_FB(36) HML_WL_FB(40) HML_WL_FB(44) HML_WL_FB(48) HML_WL_FB(52) HML_WL_FB(56)
            HML_WL_FB(60) HML_WL_FB(64)
            default: return set_err(HML_ERR_HIP, "internal error: a model of this many states on the path for more than 16");
        }
#undef HML_WL_FB
    } else {
        {
            ProfScope ps(c, "stats_emission");
            hipLaunchKernelGGL(hml_k_wide_emission, dim3(grid_for(hint, 256, 1, 4096)), dim3(256), 0, s, c->d_mdl, c->d_starts, c->d_bstat,
                               c->d_em, c->d_gsc, mix, eprobe_of(c));
        }
        if (mix) hipLaunchKernelGGL(hml_k_wide_mixture, dim3(grid_for(hint, 256, 1, 16384)), dim3(256), 0, s, c->d_mdl, c->d_em, c->d_q);
        else {
            hipLaunchKernelGGL(hml_k_wide_uniforms, dim3(grid_for((hint + 1u) / 2u, 256, 1, 4096)), dim3(256), 0, s, c->d_mdl, c->d_cdraws);
            if (p.KC == 32) launch_chunked_fb<32, hml_dev_exp, true>(c, s, p.C, ch, aprobe_of(c));
            else launch_chunked_fb<64, hml_dev_exp, true>(c, s, p.C, ch, aprobe_of(c));
        }
    }
    {
        ProfScope ps(c, "counts");
        hipLaunchKernelGGL(hml_k_wide_counts, dim3(HML_REDUCE_GROUPS), dim3(256), 0, s, c->d_q, c->d_starts, c->d_bstat, c->d_mdl, c->d_partial, c->d_wacc.as<hml_wide_acc>());
    }
    if (record) { if (int r = launch_marginals(c, s, hint, /*bracket*/ false)) return r; }
    {
        ProfScope ps(c, "params");
        hipLaunchKernelGGL(hml_k_wide_params, dim3(1), dim3(1024), 0, s, c->d_mdl, c->d_partial, c->d_wacc.as<hml_wide_acc>(), 0);
    }
    if (record) { if (int r = launch_recorders(c, s, hint)) return r; }   // (after the update: hml_k_levels.h)
    launch_history(c, method);   // (the sweep's row, where the chain keeps a history: hml_k_history.h)
    KLAUNCH_CHECK();
    return 0;
}

// ---- the two paths behind their tables (hml_ktab, hml_capi_shared.hpp); neither is batched (many_eligible refuses both modes)
static void params_compat(hml_ctx* c, int mode) {   // (draws from the reference's engine, c->d_mt)
    hipLaunchKernelGGL(hml_k_compat_draw, dim3(1), dim3(64), 0, c->stream, c->d_mdl, c->d_mt.as<hml_mt_state>(), mode);
}
static void derive_compat(hml_ctx* c) { hipLaunchKernelGGL(hml_k_compat_derive, dim3(1), dim3(64), 0, c->stream, c->d_mdl); }   // (glibc's logf)
static void params_wide(hml_ctx* c, int mode) {
    hipLaunchKernelGGL(hml_k_wide_params, dim3(1), dim3(1024), 0, c->stream, c->d_mdl, c->d_partial, c->d_wacc.as<hml_wide_acc>(), mode);
}
static void derive_wide(hml_ctx* c) { hipLaunchKernelGGL(hml_k_wide_derive, dim3(1), dim3(64), 0, c->stream, c->d_mdl); }
// (not `const`: see the per-K tables, hml_sweep.hip)
static hml_ktab hml_ktab_compat = {&sweep_compat, nullptr, &params_compat, &derive_compat, &alloc_sweep_compat};
static hml_ktab hml_ktab_wide = {&sweep_wide, nullptr, &params_wide, &derive_wide, &alloc_sweep_wide};
static const hml_ktab* rtk_tab(bool wide) { return wide ? &hml_ktab_wide : &hml_ktab_compat; }

#endif

// libhammlet_hip.so - the sweep for K states (one object per K: -DHML_TU_K=k, hammlet_amd/build.py): the kernels templated
// on the number of states and the host code that launches them, behind a table of function pointers (hml_ktab) that the
// core (hml_capi.hip) calls.  Reference: one Gibbs iteration, sampleHMM src/HMM.hpp:99-121 with
// StateSequence<ForwardBackward>::sample src/StateSequence/ForwardBackward.hpp:16-213 or <Mixture> Mixture.hpp:31-144.
#include "hml_capi_shared.hpp"

// Resident workgroups of a kernel of `threads` threads: occupancy x compute units, times `scale` (the trellis pass counts
// wavefronts, HML_TR2_WAVES to a workgroup).  Asked once and kept in *slots (0: not asked yet, -1: unknown); the environment
// variable `env` overrides it, in the same unit (tests: larger tiles / an oversized grid).
template <class Kernel>
static int resident_workgroups(const hml_ctx* c, Kernel kernel, int threads, int scale, const char* env, int* slots) {
    if (*slots == 0) {
        int per_cu = 0, cus = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, threads, 0) == hipSuccess &&
            hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device) == hipSuccess && per_cu > 0 && cus > 0)
            *slots = per_cu * cus * scale;
        else { (void)hipGetLastError(); *slots = -1; }
        if (const char* e = getenv(env)) *slots = atoi(e);
    }
    return *slots;
}

// Tiles of the block kernels that walk the trace in batches of 2^17 positions: `sub` batches per workgroup, `wg` workgroups;
// fits: within what the kernels take (HML_FUSED_MAX_SUB).
// `sub` given (> 0), or else the smallest with which at most `slots` workgroups cover the trace (no slots: it does not fit).
struct hml_tiling { uint32_t sub, wg; bool fits; };
static hml_tiling tiles_for(uint64_t T, int64_t slots, uint64_t sub = 0) {
    if (sub == 0 && slots <= 0) return {0u, 0u, false};
    const uint64_t batches = (T + HML_FUSED_SUB_POSITIONS - 1) / HML_FUSED_SUB_POSITIONS;
    if (sub == 0) sub = (batches + (uint64_t)slots - 1) / (uint64_t)slots;
    return {(uint32_t)sub, (uint32_t)((T + sub * HML_FUSED_SUB_POSITIONS - 1) / (sub * HML_FUSED_SUB_POSITIONS)), sub <= HML_FUSED_MAX_SUB};
}

// Tile size and grid of the fused block kernel: the smallest number of 2^17-position batches per workgroup with which
// the whole grid is resident at once (the workgroups wait for lower-numbered ones inside the launch).  It does not fit when
// even the largest tile is too small: those traces take the scan + scatter launches.
template <int KK>
static hml_tiling fused_geometry(hml_ctx* c) {
    return tiles_for(c->T, resident_workgroups(c, hml_k_blocks_fused<KK>, HML_FUSED_WAVES * 64, 1, "HML_FUSED_SLOTS", &c->fused_slots));
}

// what the stages of one sweep share: its plan and the pointers that follow from it
struct hml_sweep_env {
    hipStream_t s;
    hml_sweep_plan plan;
    float* gsc_plane;                  // the plane of rescale factors (none: strongly compressed sweeps, hml_sweep_plan.h)
    const uint32_t* starts_for_maps;   // ... the backward maps then apply the factor where they read a row
    float *ep, *ap;                    // probes of the emission terms / forward rows (none unless enabled)
};

// The block count of the sweep sizes the grids and picks the forward geometry, and the host only knows the count of
// an earlier sweep (it enqueues far ahead of the device).  Right after the parameters were replaced that count
// means nothing - the first sweeps of a weakly compressed chain then ran in the geometry of a strongly compressed
// one (177 ms instead of 19 ms each on C5, for as many sweeps as were enqueued at once) - so the block structure is
// enumerated once ahead of the sweep and waited for.
static int enumerate_if_stale(hml_ctx* c) {
    if (c->hint_stale && (c->dynamic || !c->blocks_valid) && !capturing(c->stream)) {
        launch_compact_pair(c, 0, 0.0f);
        KLAUNCH_CHECK();
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    c->hint_stale = false;
    return 0;
}

// The block structure: the fused block kernel where the plan wants it and its tile fits a resident grid (true: it made the
// emission terms as well), else the scan + scatter pair.
template <int KK>
static bool launch_blocks(hml_ctx* c, const hml_sweep_env& e) {
    hml_tiling t = {0u, 0u, false};
    if (e.plan.fused_wanted && (t = fused_geometry<KK>(c)).fits) {
        // K4 + K5 + K6a in one launch (hml_k_blocks_fused.h)
        ProfScope ps(c, "blocks_compact", 1);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_k_blocks_fused<KK>), dim3(t.wg), dim3(HML_FUSED_WAVES * 64), 0, e.s, c->d_summary, c->d_w, c->d_ia,
                           (uint32_t)c->T, c->d_mdl, c->key_base, c->d_group_word, c->d_stage, c->d_starts, c->d_bstat, c->d_em,
                           e.gsc_plane, e.ep, e.plan.mix ? 1 : 0, e.plan.lay, c->d_hB, t.sub, c->fused_spin_limit, c->d_dbg, c->d_mdl);
        return true;
    }
    launch_compact_pair(c, 0, 0.0f);
    return false;
}

// Emission terms per block; STATS: with the block statistics, right behind the scan + scatter pair.
template <int KK, bool STATS>
static void launch_emission(hml_ctx* c, const hml_sweep_env& e, uint32_t hint) {
    ProfScope ps(c, STATS ? "stats_emission" : "emission");
    const int mix = e.plan.mix ? 1 : 0;
    if (c->D > 1)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_k_emission_mv<KK, STATS>), dim3(grid_for(hint, 256, 64, 16384)), dim3(256), 0, e.s,
                           c->d_ia, c->d_starts, c->d_mdl, c->d_bstat, c->d_em, e.gsc_plane, e.ep, mix, e.plan.lay);
    else if (e.plan.many_blocks && e.plan.L <= hml_emit_tile<KK>::MAXL)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_k_emission_tiled<KK, STATS>), dim3(grid_for(hint, hml_emit_tile<KK>::BLOCKS, 64, 65536)),
                           dim3(256), 0, e.s, c->d_ia, c->d_starts, c->d_mdl, c->d_bstat, c->d_em, e.gsc_plane, e.ep, mix, e.plan.lay);
    else if constexpr (STATS)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_k_stats_emission<KK>), dim3(grid_for(hint, 256, 64, 16384)), dim3(256), 0, e.s,
                           c->d_ia, c->d_starts, c->d_mdl, c->d_bstat, c->d_em, e.gsc_plane, e.ep, mix, e.plan.lay);
    else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_k_emission<KK>), dim3(grid_for(hint, 256, 64, 16384)), dim3(256), 0, e.s, c->d_bstat, c->d_starts, c->d_mdl,
                           c->d_em, e.gsc_plane, e.ep, mix, e.plan.lay);
}

// Weakly compressed univariate FB sweeps: emission terms, filter and candidate maps fused per tile, repair, chain and states
// (hml_k_trellis.h, hml_k_trellis_rows.h).
template <int KK>
static void launch_trellis(hml_ctx* c, const hml_sweep_env& e, uint32_t hint) {
    hipStream_t s = e.s;
    // chunk length by the number of blocks: the warm-up (emission terms included) is paid once per chunk, and a
    // wavefront takes 64 chunks - long chunks where there are enough blocks to fill the machine with wavefronts anyway
    bool measure = false;
    const bool rows = c->knobs.tre_rows;
    if (rows)   // wavefront slots of the first pass on this device (asked once)
        (void)resident_workgroups(c, hml_k_trellis_rows<KK, false>, 64 * HML_TR2_WAVES, HML_TR2_WAVES, "HML_TRELLIS_SLOTS", &c->tre_slots);
    const uint32_t TL = tre_pick_L(c, hint, capturing(s), &measure);
    hipEvent_t tev0 = nullptr, tev1 = nullptr;
    if (measure) { tev0 = ev_get(c); tev1 = ev_get(c); hipEventRecord(tev0, s); }
    if (c->tre_last_L != TL && getenv("HML_TRELLIS_TUNE_DEBUG")) fprintf(stderr, "[trellis] chunk length %u for %u blocks (%d wavefront slots)\n", TL, hint, c->tre_slots);
    c->tre_last_L = TL;
    const uint64_t tchunks = ((uint64_t)hint + TL - 1) / TL;
    const uint64_t tgroups = (tchunks + HML_TRE_NCH - 1) / HML_TRE_NCH;
    float *const ep = e.ep, *const ap = e.ap;
    {
        ProfScope ps(c, "trellis", 1);
        if (e.plan.first_pass == HML_PASS_ROWS_SINGLE)
            hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_k_trellis_rows<KK, true>), dim3(grid_for(tgroups, HML_TR2_WAVES, 4, 1 << 20)), dim3(64 * HML_TR2_WAVES), 0, s,
                               c->d_ia, c->d_starts, c->d_mdl, c->d_mdl, c->d_bstat, c->d_smap, c->d_cmap, c->d_entry, c->d_exitA, c->d_fb, ep, ap, c->d_tre_ckpt, TL);
        else if (e.plan.first_pass == HML_PASS_ROWS)
            hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_k_trellis_rows<KK, false>), dim3(grid_for(tgroups, HML_TR2_WAVES, 4, 1 << 20)), dim3(64 * HML_TR2_WAVES), 0, s,
                               c->d_ia, c->d_starts, c->d_mdl, c->d_mdl, c->d_bstat, c->d_smap, c->d_cmap, c->d_entry, c->d_exitA, c->d_fb, ep, ap, c->d_tre_ckpt, TL);
        else
            hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_k_trellis_tile<KK>), dim3(grid_for(tgroups, 1, 16, 1 << 20)), dim3(64), 0, s,
                               c->d_ia, c->d_starts, c->d_mdl, c->d_mdl, c->d_bstat, c->d_smap, c->d_cmap, c->d_entry, c->d_exitA, c->d_fb, ep, ap, TL);
    }
    {
        // verification, rounds of parallel refits from the predecessors' end vectors (two by default, hml_ctx.hpp; the lists of stale chunks
        // alternate between d_redo and d_redo2), then the sequential finisher: each exits at once when its list is empty
        ProfScope ps(c, "trellis_repair");
        hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_k_trellis_verify<KK>), dim3(grid_for(tchunks, 256, 16, 1 << 14)), dim3(256), 0, s, c->d_mdl,
                           c->d_entry, c->d_exitA, c->d_redo, TL);
        int in_a = 1;
        for (uint32_t round = 0; round < c->tre_refit_rounds; ++round, in_a ^= 1) {
            uint32_t* lin = in_a ? c->d_redo : c->d_redo2;
            uint32_t* lout = in_a ? c->d_redo2 : c->d_redo;
            hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_k_trellis_refit<KK>), dim3(4096), dim3(64), 0, s, c->d_ia, c->d_starts, c->d_mdl, c->d_smap,
                               c->d_cmap, c->d_entry, c->d_exitA, c->d_fb, ep, ap, lin, in_a, (rows && c->tre_ckpt) ? c->d_tre_ckpt : nullptr, TL);
            hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_k_trellis_verify_list<KK>), dim3(64), dim3(256), 0, s, c->d_mdl, c->d_entry, c->d_exitA,
                               lin, lout, c->d_touched, in_a, round, TL);
        }
        hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_k_trellis_serial<KK>), dim3(1), dim3(256), 0, s, c->d_ia, c->d_starts, c->d_mdl, c->d_smap,
                           c->d_cmap, c->d_entry, c->d_exitA, c->d_fb, ep, ap, in_a ? c->d_redo : c->d_redo2, in_a, c->d_tre_bitmap, TL);
    }
    {
        ProfScope ps(c, "backward_chain");
        const uint64_t supers = (tchunks + 63) / 64;
        hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_k_trellis_super<KK>), dim3(grid_for(supers * 64, 256, 16, 1 << 16)), dim3(256), 0, s, c->d_cmap,
                           c->d_mdl, c->d_scmap, c->d_super, TL);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_k_trellis_chain<KK>), dim3(1), dim3(1024), 0, s, c->d_super, c->d_mdl, c->d_bentry2, TL);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_k_trellis_states<KK>), dim3(grid_for(tgroups, 1, 16, 1 << 20)), dim3(64), 0, s, c->d_smap,
                           c->d_scmap, c->d_bentry2, c->d_mdl, c->d_q, TL);
    }
    if (measure) {
        // a measuring sweep (a few per chain): wait for the trellis kernels and note what this chunk length cost
        hipEventRecord(tev1, s);
        float ms = 0.0f;
        const bool ok = hipEventSynchronize(tev1) == hipSuccess && hipEventElapsedTime(&ms, tev0, tev1) == hipSuccess;
        c->ev_pool.push_back(tev0);
        c->ev_pool.push_back(tev1);
        if (ok) tre_tune_report(c, hint, ms); else { (void)hipGetLastError(); c->tre_autotune = false; }
    }
    c->tre_dense_sweeps++;
}

// Forward filter over chunks, backward maps, the chain over the chunk maps (one level, or two where there are many blocks).
template <int KK>
static void launch_forward_backward(hml_ctx* c, const hml_sweep_env& e, uint32_t hint) {
    hipStream_t s = e.s;
    const int L = e.plan.L;
    const hml_layout lay = e.plan.lay;
    const uint64_t chunks = ((uint64_t)hint + L - 1) / L;
    const int gF = grid_for(chunks, HML_FWD_THREADS, 16, 1 << 20);
    {
        ProfScope ps(c, "forward");
        hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_k_forward<KK>), dim3(gF), dim3(HML_FWD_THREADS), 0, s, c->d_em, e.gsc_plane, c->d_mdl, c->d_rows,
                           e.ap, c->d_entry, c->d_exitA, c->d_fb, L, lay);
    }
    // backward maps (verifies the forward chunks on the way), then one workgroup: repair if a check failed,
    // and the chain over the chunk maps
    const uint64_t bch = ((uint64_t)hint + HML_BWD_CHUNK - 1) / HML_BWD_CHUNK;
    {
        ProfScope ps(c, "backward_maps");
        hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_k_backward_maps<KK>), dim3(grid_for(bch * 64, HML_BWD_MAPS_THREADS, 16, 1 << 18)), dim3(HML_BWD_MAPS_THREADS), 0,
                           s, c->d_rows, c->d_mdl, c->d_smap, c->d_cmap, lay, c->d_entry, c->d_exitA, c->d_redo, L, e.starts_for_maps, c->d_mdl);
    }
    ProfScope ps(c, "backward_chain");
    auto chain = [&](unsigned long long* maps, uint8_t* entries, int steps, int level) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_k_backward_chain<KK>), dim3(1), dim3(1024), 0, s, maps, c->d_mdl, entries, c->d_em, e.gsc_plane, c->d_rows, e.ap,
                           c->d_entry, c->d_exitA, c->d_fb, c->d_redo, c->d_touched, c->d_smap, L, lay, steps, level, e.starts_for_maps);
    };
    if (!e.plan.many_blocks) return chain(c->d_cmap, c->d_bentry, 3, 0);
    // millions of backward chunks: repair step alone, then the two-level chain
    chain(c->d_cmap, c->d_bentry, 1, 0);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_k_backward_super<KK>), dim3(grid_for(bch, 256, 16, 1 << 16)), dim3(256), 0, s, c->d_cmap, c->d_mdl, c->d_scmap, c->d_super);
    chain(c->d_super, c->d_bentry2, 2, 1);
    hipLaunchKernelGGL(hml_k_backward_entries, dim3(grid_for(bch, 256, 16, 1 << 16)), dim3(256), 0, s, c->d_scmap, c->d_bentry2, c->d_mdl, c->d_bentry,
                       (uint32_t)hml_mapfmt<KK>::BITS);
}

// Sufficient statistics of the sweep's states.  MAPS: the states are still packed in the backward maps (the forward-backward
// path); the trellis path and mixture sweeps have written them out.
template <int KK, bool MAPS>
static void launch_counts(hml_ctx* c, hipStream_t s, int variant) {
    ProfScope ps(c, "counts");
    const unsigned long long* const smap = MAPS ? c->d_smap.get() : nullptr;
    const uint8_t* const bentry = MAPS ? c->d_bentry.get() : nullptr;
    if (variant == HML_COUNTS_MV)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_k_counts<KK, MAPS, true>), dim3(HML_REDUCE_GROUPS), dim3(256), 0, s, c->d_q,
                           c->d_starts, c->d_bstat, c->d_mdl, c->d_partial, smap, bentry);
    else if (variant == HML_COUNTS_DENSE)   // hundreds of chunks per workgroup: one wavefront per chunk (same tree, bit for bit)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_k_counts_dense<KK, MAPS>), dim3(HML_REDUCE_GROUPS), dim3(256), 0, s, c->d_q,
                           c->d_starts, c->d_bstat, c->d_mdl, c->d_partial, smap, bentry);
    else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_k_counts<KK, MAPS>), dim3(HML_REDUCE_GROUPS), dim3(256), 0, s, c->d_q,
                           c->d_starts, c->d_bstat, c->d_mdl, c->d_partial, smap, bentry);
}

// One sweep of the default path.  The device writes the block count (h_B[0]) while the host enqueues: the plan is fixed from
// the first read of it, the grids follow the later ones.
template <int KK>
static int sweep_k(hml_ctx* c, char method, bool record) {
    if (int r = enumerate_if_stale(c)) return r;
    refresh_hint(c);
    // (the fused block kernel reported a bounded wait that expired - someone else is using the GPU, h_B[1]: not again)
    const bool wait_expired = c->h_B[1] != 0u;
    if (wait_expired && !c->knobs.fused_keep && (c->dynamic || !c->blocks_valid)) c->knobs.fused_blocks = false;
    const hml_sweep_plan plan = plan_of(c, method == HML_METHOD_MIXTURE, wait_expired);
    const hml_sweep_env e = {c->stream, plan, plan.keep_gsc ? c->d_gsc.get() : nullptr, plan.keep_gsc ? nullptr : c->d_starts.get(), eprobe_of(c), aprobe_of(c)};
    // block structure and, unless the block kernel or the trellis pass makes them, emission terms
    bool emitted = false;
    if (c->dynamic || !c->blocks_valid) {
        const bool fused = launch_blocks<KK>(c, e);
        if (!fused && !plan.trellis) { refresh_hint(c); launch_emission<KK, true>(c, e, grid_hint(c)); }
        KLAUNCH_CHECK();
        emitted = true;
        if (!c->dynamic) c->blocks_valid = true;
    }
    refresh_hint(c);
    const uint32_t hint = grid_hint(c);
    if (!emitted && !plan.trellis) launch_emission<KK, false>(c, e, hint);
    // states
    if (plan.trellis) {
        launch_trellis<KK>(c, e, hint);
        launch_counts<KK, false>(c, e.s, HML_COUNTS_DENSE);
    } else if (!plan.mix) {
        launch_forward_backward<KK>(c, e, hint);
        launch_counts<KK, true>(c, e.s, plan.counts);
    } else {
        {
            ProfScope ps(c, "mixture");
            hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_k_mixture<KK>), dim3(grid_for(hint, 256, 64, 16384)), dim3(256), 0, e.s, c->d_em, c->d_mdl, c->d_q, plan.lay);
        }
        launch_counts<KK, false>(c, e.s, plan.counts);
    }
    if (record) { if (int r = launch_marginals(c, e.s, hint, /*bracket*/ true)) return r; }
    {
        ProfScope ps(c, "params");
        if (plan.params_spread) hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_k_params_spread<KK>), dim3(HML_PARAMS_TREE_WGS), dim3(1024), 0, e.s, c->d_mdl, c->d_partial);
        else hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_k_params<KK>), dim3(1), dim3(1024), 0, e.s, c->d_mdl, c->d_partial, 0);
    }
    if (record) { if (int r = launch_recorders(c, e.s, hint)) return r; }   // (after the update: hml_k_levels.h)
    launch_history(c, method);   // (the sweep's row, where the chain keeps a history: hml_k_history.h)
    KLAUNCH_CHECK();
    return 0;
}


// How a batch of chains is launched (iterate_many_k): its groups, the block path, the tiles of the many-chain block kernels.
struct hml_many_geometry {
    int G = 1;
    struct { int first, count; hipStream_t s; } grp[4];
    bool fm = false;                 // the chains read ONE trace: the many-chain block kernels
    bool fm_split = true;            // ... the two launches that no workgroup waits in, not the fused kernel
    hml_tiling fs = {1u, 0u, true}, fmt = {0u, 0u, false};   // tiles of the split / the fused many-chain kernels
    uint64_t fs_tiles1 = 0;          // tiles of one batch: what the per-tile arrays are sized for
};
template <int KK>
static hml_many_geometry many_geometry(hml_ctx* const* cs, int n) {
    hml_ctx* c0 = cs[0];
    hml_many_geometry m;
    // The batch runs as G GROUPS of chains, each on a stream of its own (its first chain's), enqueued by this one host thread: a
    // group's latency-bound stretches - the one-workgroup kernels, the block kernel's hand-off, launch boundaries - are filled by
    // the other group's throughput-bound kernels (round 4, config 3, ms per round of sweeps: 2 chains 0.078 against 0.082, 4: 0.106 /
    // 0.126, 8: 0.158 / 0.174, 16: 0.259 / 0.307).  More than two groups lose again: the block kernel's pass over the summary and
    // the weights does not depend on the number of chains and is repeated per group, on tiles that grow with the number of grids
    // that have to be resident together (8 chains in 4 groups: 0.236).  HML_MANY_GROUPS overrides.
    m.G = n >= 2 ? 2 : 1;
    if (const char* e = getenv("HML_MANY_GROUPS")) m.G = std::max(1, std::min(std::min(atoi(e), 4), n));
    for (int g = 0; g < m.G; ++g) {
        m.grp[g].first = (int)((int64_t)g * n / m.G);
        m.grp[g].count = (int)((int64_t)(g + 1) * n / m.G) - m.grp[g].first;
        m.grp[g].s = cs[m.grp[g].first]->stream;
    }
    // Chains attached to ONE trace (hml_attach_observations) take the many-chain block kernel: block starts, statistics and
    // emission terms of every chain from one pass over the shared summary / weights / integral array (hml_k_blocks_fused_many.h).
    // Its workgroups wait for lower-numbered ones inside the launch, so the whole grid must be resident - the tile grows
    // with the trace like the single-chain kernel's (fused_geometry).
    m.fm = c0->trace != nullptr && c0->knobs.fused_blocks;
    for (int k = 0; k < n; ++k) m.fm = m.fm && cs[k]->trace == c0->trace && cs[k]->knobs.fused_blocks && cs[k]->key_base == c0->key_base;
    // HML_FM_SPLIT (default 1): the block structure of attached chains in two launches that no workgroup waits in
    // (hml_k_blocks_split_many.h) instead of the fused kernel; tiles of 2^17 positions (more per tile only beyond 4096 tiles)
    if (const char* e = getenv("HML_FM_SPLIT")) m.fm_split = atoi(e) != 0;
    m.fs_tiles1 = (c0->T + HML_FUSED_SUB_POSITIONS - 1) / HML_FUSED_SUB_POSITIONS;
    m.fs = tiles_for(c0->T, 4096);
    if (const char* e = getenv("HML_FM_SPLIT_SUB")) m.fs = tiles_for(c0->T, 0, (uint64_t)std::max(1, atoi(e)));   // (tests: tiles of several batches)
    if (!m.fs.fits) m.fm_split = false;
    if (m.fm && !m.fm_split) {
        const int fm_slots = resident_workgroups(c0, hml_m_blocks_fused<KK>, HML_FUSED_WAVES * 64, 1, "HML_FUSED_MANY_SLOTS", &c0->fm_slots);
        // The block kernels of the G groups run side by side, and other contexts of the device that are not in this batch may be
        // running a batch of their own at the same time (another host thread): every launch takes its SHARE of the workgroup
        // slots, so that all these grids are resident together.
        const int live = c0->device < 64 ? g_live_ctx[c0->device].load() : n;
        const int sharers = m.G * std::max(1, (live + n - 1) / n);
        m.fmt = tiles_for(c0->T, fm_slots > 0 ? std::max<int64_t>(1, fm_slots / sharers) : 0);
        if (!m.fmt.fits) m.fm = false;
    }
    return m;
}

template <int KK>
static int iterate_many_k(hml_ctx* const* cs, int n, uint64_t first, uint64_t iterations, uint64_t thinning, uint64_t* done) {
    hml_ctx* c0 = cs[0];
    hipStream_t s = c0->stream;
    const uint32_t T = (uint32_t)c0->T;
    const int L = c0->knobs.geo[HML_GEO_MANY].L;   // (the layouts are the chains' own: their strides follow their block capacities)
    const int with_gsc = c0->knobs.late_rescale ? 0 : 1;
    const uint32_t n_groups = (c0->n_spans + HML_GROUP_SPANS - 1) / HML_GROUP_SPANS;
    const bool records = thinning > 0 && thinning <= iterations;
    unsigned long long rec_mask = 0ull;
    for (int i = 0; i < n; ++i) {
        if (records) { if (int r = ensure_recorders(cs[i])) return r; }
        if (int r = pooled_refusal(cs[i], records, "a context")) return r;
        if (records && cs[i]->rec_marginals) {
            if (int r = ensure_marginal_buffers(cs[i])) return r;
            rec_mask |= 1ull << i;
        }
    }
    // the chains' pointers, in device memory of chain 0 (kept for the next call)
    std::vector<hml_chain_dev> h(n);
    for (int i = 0; i < n; ++i) {
        hml_ctx* c = cs[i];
        hml_chain_dev& d = h[i];
        d.summary = c->d_summary; d.w = c->d_w; d.ia = c->d_ia; d.key_base = c->key_base; d.n_spans = c->n_spans;
        d.stage = c->d_stage; d.span_count = c->d_span_count; d.coarse1 = c->d_coarse1; d.starts = c->d_starts; d.host_B = c->d_hB;
        d.bstat = c->d_bstat; d.mdl = c->d_mdl; d.em = c->d_em; d.gsc = c->d_gsc; d.rows = c->d_rows; d.entry = c->d_entry; d.exitv = c->d_exitA;
        d.fb = c->d_fb; d.redo = c->d_redo; d.touched = c->d_touched; d.smap = c->d_smap; d.cmap = c->d_cmap; d.bentry = c->d_bentry;
        d.q = c->d_q; d.partial = c->d_partial; d.diff = c->d_diff; d.boundary = c->d_boundary; d.lay = c->knobs.geo[HML_GEO_MANY].lay;
    }
    if (c0->many_cap < n) {
        c0->many_cap = 0;
        HIPCHK(c0->d_many.alloc(n * sizeof(hml_chain_dev)));
        c0->many_cap = n;
    }
    HIPCHK(hipMemcpyAsync(c0->d_many.get(), h.data(), n * sizeof(hml_chain_dev), hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));   // (the staging vector goes out of scope below)
    const hml_chain_dev* d_cs = c0->d_many.as<const hml_chain_dev>();
    hml_many_geometry m = many_geometry<KK>(cs, n);
    // every chain's own stream goes on behind its group's (also on the early ways out)
    auto join = [&](bool wait) -> int {
        for (int g = 0; g < m.G; ++g) {
            if (wait) { HIPCHK(hipStreamSynchronize(m.grp[g].s)); continue; }
            hipEvent_t ev = ev_get(c0);
            HIPCHK(hipEventRecord(ev, m.grp[g].s));
            for (int k = m.grp[g].first; k < m.grp[g].first + m.grp[g].count; ++k) if (cs[k]->stream != m.grp[g].s) HIPCHK(hipStreamWaitEvent(cs[k]->stream, ev, 0));
            c0->ev_pool.push_back(ev);
        }
        return 0;
    };
    for (uint64_t i = first; i < iterations; ++i) {
        // a chain left the strongly compressed regime, or halted because its blocks outgrew its buffers (hml_state.h): back to the caller
        for (int k = 0; k < n; ++k) if (!many_sparse(cs[k]) || chain_halted(cs[k])) { *done = i; return join(true); }
        const bool record = thinning > 0 && ((i + 1) % thinning == 0);
        for (int k = 0; k < n; ++k) log_sweep(cs[k], HML_METHOD_FB, record);
        // (a bounded wait of the block kernel expired - somebody else is using the GPU: the scan + scatter launches from here on)
        if (m.fm) for (int k = 0; k < n; ++k) if (cs[k]->h_B[1] && !cs[k]->knobs.fused_keep) m.fm = false;
        for (int g = 0; g < m.G; ++g) {
            const int g0 = m.grp[g].first, gn = m.grp[g].count;
            hipStream_t s = m.grp[g].s;
            const hml_chain_dev* d_g = d_cs + g0;
            uint32_t hint = 0;
            for (int k = g0; k < g0 + gn; ++k) hint = std::max(hint, grid_hint(cs[k]));
            const unsigned ny = (unsigned)gn;
            const unsigned gB = (unsigned)grid_for(hint, 256, 64, 16384);
            if (m.fm && m.fm_split) {
                // two launches without a wait between workgroups (hml_k_blocks_split_many.h): the chains' block starts, then
                // statistics and emission terms - up to sixteen chains to a launch
                for (int k0 = g0; k0 < g0 + gn; k0 += HML_FS_MAX_CHAINS) {
                    const int nk = std::min(g0 + gn - k0, (int)HML_FS_MAX_CHAINS);
                    hml_fs_args fa;
                    memset(&fa, 0, sizeof fa);
                    for (int k = 0; k < nk; ++k) {
                        hml_ctx* c = cs[k0 + k];
                        hml_fs_chain& f = fa.c[k];
                        const hml_wave_total_layout wt = hml_layout_wave_total(c->d_wave_total.get(), m.fs_tiles1);
                        f.mdl = c->d_mdl; f.group_word = c->d_group_word; f.wave_total = wt.wave_total; f.stage = c->d_stage; f.starts = c->d_starts;
                        f.tile_before = wt.tile_before; f.tile_prev = wt.tile_prev;
                        f.bstat = c->d_bstat; f.em = c->d_em; f.gsc = with_gsc ? c->d_gsc : nullptr; f.host_words = c->d_hB; f.lay = c->knobs.geo[HML_GEO_MANY].lay;
                    }
                    hipLaunchKernelGGL(hml_m_blocks_list, dim3(m.fs.wg), dim3(HML_FUSED_WAVES * 64), 0, s, c0->d_summary, c0->d_w, T, c0->key_base, fa, nk, m.fs.sub);
                    hipLaunchKernelGGL(hml_m_blocks_offsets, dim3(1, (unsigned)nk), dim3(1024), 0, s, fa, m.fs.wg, m.fs.sub);
                    hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_m_blocks_emit<KK>), dim3(m.fs.wg), dim3(HML_FUSED_WAVES * 64), 0, s, c0->d_ia, T, fa, nk, m.fs.sub);
                }
            } else if (m.fm) {
                for (int k0 = g0; k0 < g0 + gn; k0 += HML_FM_MAX_CHAINS) {
                    const int nk = std::min(g0 + gn - k0, (int)HML_FM_MAX_CHAINS);
                    hml_fm_args fa;
                    memset(&fa, 0, sizeof fa);
                    for (int k = 0; k < nk; ++k) {
                        hml_ctx* c = cs[k0 + k];
                        hml_fm_chain& f = fa.c[k];
                        f.mdl = c->d_mdl; f.group_word = c->d_group_word; f.stage = c->d_stage; f.starts = c->d_starts; f.bstat = c->d_bstat;
                        f.em = c->d_em; f.gsc = with_gsc ? c->d_gsc : nullptr; f.host_words = c->d_hB; f.lay = c->knobs.geo[HML_GEO_MANY].lay;
                    }
                    hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_m_blocks_fused<KK>), dim3(m.fmt.wg), dim3(HML_FUSED_WAVES * 64), 0, s, c0->d_summary, c0->d_w, c0->d_ia,
                                       T, c0->key_base, fa, nk, m.fmt.sub, c0->fused_spin_limit, g == 0 ? c0->d_dbg : nullptr);
                }
            } else {
                hipLaunchKernelGGL(hml_m_compact_scan_summary, dim3(n_groups, ny), dim3(256), 0, s, d_g, T);
                hipLaunchKernelGGL(hml_m_compact_scatter, dim3(n_groups, ny), dim3(256), 0, s, d_g, T);
                hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_m_stats_emission<KK>), dim3(gB, ny), dim3(256), 0, s, d_g, with_gsc);
            }
            const uint64_t chunks = ((uint64_t)hint + L - 1) / L;
            const uint64_t bch = ((uint64_t)hint + HML_BWD_CHUNK - 1) / HML_BWD_CHUNK;
            // the chains' pointers travel as a kernel argument, up to sixteen chains to a launch (hml_many_args)
            for (int k0 = g0; k0 < g0 + gn; k0 += HML_MANY_ARG_CHAINS) {
                const int nk = std::min(g0 + gn - k0, (int)HML_MANY_ARG_CHAINS);
                hml_many_args ma;
                memset(&ma, 0, sizeof ma);
                for (int k = 0; k < nk; ++k) ma.c[k] = h[k0 + k];
                const unsigned nyk = (unsigned)nk;
                hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_m_forward<KK>), dim3((unsigned)grid_for(chunks, HML_FWD_THREADS, 16, 1 << 20), nyk), dim3(HML_FWD_THREADS), 0, s, ma, with_gsc, L);
                hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_m_backward_maps<KK>), dim3((unsigned)grid_for((bch + 1) / 2 * 64, HML_BWD_MAPS_THREADS, 16, 1 << 18), nyk), dim3(HML_BWD_MAPS_THREADS), 0, s, ma, with_gsc, L);   // (a wavefront per two chunks)
                hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_m_backward_chain<KK>), dim3(1, nyk), dim3(1024), 0, s, ma, with_gsc, L);
                hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_m_counts<KK>), dim3(HML_REDUCE_GROUPS, nyk), dim3(256), 0, s, ma);
                if (record && (rec_mask >> k0)) hipLaunchKernelGGL(hml_m_record, dim3(gB, nyk), dim3(256), 0, s, ma, rec_mask >> k0);
                hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_m_params<KK>), dim3(HML_PARAMS_TREE_WGS, nyk), dim3(1024), 0, s, ma);
            }
            // the chains' own recordings (levels, breaks, bands): one launch each behind the batch's parameter kernels
            if (record) for (int kind = 0; kind < HML_REC_KINDS; ++kind)
                for (int k = g0; k < g0 + gn; ++k) if (cs[k]->rec[kind].on) launch_record_kernel(cs[k], kind, s, dim3(gB));
            if (record) for (int k = g0; k < g0 + gn; ++k) if (cs[k]->rg.on) launch_region_kernels(cs[k], s, hint, /*bracket*/ false);   // (and their regions: hml_k_regions.h)
            for (int k = g0; k < g0 + gn; ++k) if (history_due(cs[k])) hml_history_launch(cs[k], s, HML_METHOD_FB);   // (every sweep's row: hml_k_history.h)
        }
        KLAUNCH_CHECK();
        if (record) {
            bool any_cb = false;
            for (int k = 0; k < n; ++k) any_cb = any_cb || cs[k]->cb;
            if (any_cb) {
                if (int r = join(true)) return r;
                for (int k = 0; k < n; ++k) {
                    if (int r = check_device_error(cs[k])) return r;
                    if (cs[k]->cb && !chain_halted(cs[k])) cs[k]->cb(cs[k], i, cs[k]->cb_user);   // (a halted chain calls back when it catches up: hml_settle)
                }
            }
        }
    }
    if (int r = join(false)) return r;
    *done = iterations;
    return 0;
}



// ------------------------------------------------------------------------------------------------
// The K-dependent part behind its table (one per object: -DHML_TU_K=k; a development build: -DHML_ONLY_K=k; else all).
// (the tables are not `const`: the device pass of the compiler takes a constant with constant initialisers for a device
// constant as well and then looks for the host functions it points to; a plain host variable is only parsed there - which is
// what instantiates the kernels that sweep_k<K> launches)
// The compiler emits the kernels of K states into the code object in the order of their first use.  This list is that order as
// it was before the sweep was cut into stages (the trellis kernels between emission terms and filter, the many-chain block kernel
// ahead of the others): stating it keeps every per-K code object what it was byte for byte, whatever the host code's shape.
#define HML_KERNEL_ORDER(KK)                                                                                                       \
    [[maybe_unused]] static void hml_kt_order_##KK() {                                                                             \
        (void)hml_k_blocks_fused<KK>; (void)hml_k_emission_mv<KK, true>; (void)hml_k_emission_tiled<KK, true>; (void)hml_k_stats_emission<KK>; \
        (void)hml_k_emission_mv<KK, false>; (void)hml_k_emission_tiled<KK, false>; (void)hml_k_emission<KK>;                        \
        (void)hml_k_trellis_rows<KK, false>; (void)hml_k_trellis_rows<KK, true>; (void)hml_k_trellis_tile<KK>; (void)hml_k_trellis_verify<KK>; \
        (void)hml_k_trellis_refit<KK>; (void)hml_k_trellis_verify_list<KK>; (void)hml_k_trellis_serial<KK>; (void)hml_k_trellis_super<KK>; \
        (void)hml_k_trellis_chain<KK>; (void)hml_k_trellis_states<KK>; (void)hml_k_counts_dense<KK, false>; (void)hml_k_forward<KK>; \
        (void)hml_k_backward_maps<KK>; (void)hml_k_backward_chain<KK>; (void)hml_k_backward_super<KK>; (void)hml_k_counts<KK, true, true>; \
        (void)hml_k_counts_dense<KK, true>; (void)hml_k_counts<KK, true>; (void)hml_k_mixture<KK>; (void)hml_k_counts<KK, false, true>; \
        (void)hml_k_counts<KK, false>; (void)hml_k_params_spread<KK>; (void)hml_m_blocks_fused<KK>; (void)hml_m_blocks_emit<KK>;    \
        (void)hml_m_stats_emission<KK>; (void)hml_m_forward<KK>; (void)hml_m_backward_maps<KK>; (void)hml_m_backward_chain<KK>;     \
        (void)hml_m_counts<KK>; (void)hml_m_params<KK>;                                                                             \
    }
#define HML_DEFINE_KTAB(KK)                                                                                                        \
    static void hml_kt_params_##KK(hml_ctx* c, int mode) {                                                                         \
        hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_k_params<KK>), dim3(1), dim3(1024), 0, c->stream, c->d_mdl, c->d_partial, mode);    \
    }                                                                                                                              \
    static void hml_kt_derive_##KK(hml_ctx* c) {                                                                                   \
        hipLaunchKernelGGL(HIP_KERNEL_NAME(hml_k_derive<KK>), dim3(1), dim3(64), 0, c->stream, c->d_mdl);                          \
    }                                                                                                                              \
    HML_KERNEL_ORDER(KK)                                                                                                           \
    extern hml_ktab hml_ktab_##KK;                                                                                                 \
    hml_ktab hml_ktab_##KK = {&sweep_k<KK>, &iterate_many_k<KK>, &hml_kt_params_##KK, &hml_kt_derive_##KK, &hml_alloc_sweep_default};
#if defined(HML_TU_K)
#define HML_DEFINE_KTAB_(K) HML_DEFINE_KTAB(K)
HML_DEFINE_KTAB_(HML_TU_K)
#elif defined(HML_ONLY_K)
#define HML_DEFINE_KTAB_(K) HML_DEFINE_KTAB(K)
HML_DEFINE_KTAB_(HML_ONLY_K)
#else
HML_DEFINE_KTAB(2) HML_DEFINE_KTAB(3) HML_DEFINE_KTAB(4) HML_DEFINE_KTAB(5) HML_DEFINE_KTAB(6) HML_DEFINE_KTAB(7) HML_DEFINE_KTAB(8) HML_DEFINE_KTAB(9)
HML_DEFINE_KTAB(10) HML_DEFINE_KTAB(11) HML_DEFINE_KTAB(12) HML_DEFINE_KTAB(13) HML_DEFINE_KTAB(14) HML_DEFINE_KTAB(15) HML_DEFINE_KTAB(16)
#endif

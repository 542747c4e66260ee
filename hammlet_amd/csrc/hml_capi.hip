// libhammlet_hip.so - C ABI (include/hml.h) over the gfx950 kernels.  Host side only orchestrates:
// allocation, launches on the context's stream, and the few inherently sequential one-time steps of
// the reference's driver (noise estimate src/main.cpp:303-311, autoPrior src/AutoPriors.hpp:86-110).
#include "hml_capi_shared.hpp"

static thread_local std::string g_err;
int hml_set_err(int code, const std::string& msg) { g_err = msg; return code; }

// the table of K states, or nullptr (outside [2, 16]; a development build knows one K only: -DHML_ONLY_K=5, tools/dev_build.py)
static const hml_ktab* ktab(int K);
// ... and the tables of the two paths that take the number of states at run time (hml_rtk_sweep.hpp)
static const hml_ktab* rtk_tab(bool wide);

std::atomic<int> hml_live_ctx[64];
int hml_ctx_bind(hml_ctx* c) { return ctx_bind(c); }
int hml_ctx_fetch_model(hml_ctx* c, hml_model* out) { return fetch_model(c, out); }

// ------------------------------------------------------------------------------------------------
// hml_debug_eval: evaluates one of the shared host/device functions on the GPU (parity probe for
// hml_math.h / hml_dist.h: the tests compare with the same function compiled by gcc).
HML_KERNEL void hml_k_debug_eval(int fn, const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out,
                                 uint64_t n, uint64_t seed) {
    if (fn == 24) {   // gamma draw with ONE active lane per wavefront (divergence-free control)
        const uint64_t nw = ((uint64_t)gridDim.x * blockDim.x) >> 6;
        if ((threadIdx.x & 63) != 0) return;
        for (uint64_t i = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; i < n; i += nw) {
            hml_dev_src src;
            src.s = hml_stream_open(hml_make_key(seed, 0), HML_KIND_THETA, seed, (uint32_t)i);
            out[i] = hml_gamma_f32<hml_devmath>(src, a[i], b[i]);
        }
        return;
    }
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const float x = a[i], y = b ? b[i] : 0.0f;
        float r = 0.0f;
        switch (fn) {
            case 0: r = hml_expf(x); break;
            case 1: r = hml_logf(x); break;
            case 2: r = hml_powf_unit(x, y); break;
            case 3: r = HML_SQRTF(x); break;
            case 4: r = x / y; break;
            case 5: {   // gamma(alpha = x, beta = y) from sub-stream (THETA, epoch = seed, index = i)
                hml_dev_src src;
                src.s = hml_stream_open(hml_make_key(seed, 0), HML_KIND_THETA, seed, (uint32_t)i);
                r = hml_gamma_f32<hml_devmath>(src, x, y);
            } break;
            case 6: {   // normal(mean = x, sd = y)
                hml_dev_src src;
                src.s = hml_stream_open(hml_make_key(seed, 0), HML_KIND_PI, seed, (uint32_t)i);
                hml_normal_f32<hml_devmath> nd;
                r = nd.draw(src, x, y);
            } break;
            case 7: r = (float)hml_log((double)x); break;
            case 8: r = (float)hml_exp_nonpos((double)x); break;
            case 9: r = (float)((double)x / (double)y); break;
            case 40: r = hml_glibc_expf(x); break;            // hml_math_glibc.h: the reference-compatible mode's arithmetic
            case 41: r = hml_glibc_logf(x); break;
            case 42: r = hml_glibc_powf_unit(x, y); break;
            case 43: { const double Zd = (double)y; r = hml_tr2_quotient(x, Zd, hml_tr2_reciprocal(Zd)); } break;   // x / y through the double reciprocal (hml_k_trellis_rows.h)
            case 10: r = (float)(1.0 / (double)x); break;
            case 12: case 13: case 14: case 15: case 16: case 17: case 18: case 19: case 20: case 21: case 22: case 23: {
                hml_dev_src src; src.s = hml_stream_open(hml_make_key(seed, 0), HML_KIND_THETA, seed, (uint32_t)i);
                const float alpha = x, beta = y; (void)beta;
                const float malpha = alpha < 1.0f ? alpha + 1.0f : alpha;
                const float a1 = malpha - 1.0f / 3.0f;
                const float a2 = 1.0f / hml_devmath::sqrtf_(9.0f * a1);
                hml_normal_f32<hml_devmath> nd;
                float n = nd.draw(src, 0.0f, 1.0f);
                float v = 1.0f + a2 * n;
                float v3 = v * v * v;
                float u = hml_canonical_f32(src);
                const bool c1 = (double)u > (double)1.0f - 0.0331 * (double)n * (double)n * (double)n * (double)n;
                const bool c2 = ((double)hml_devmath::logf_(u) > (0.5 * (double)n * (double)n + (double)a1 * ((1.0 - (double)v3) + (double)hml_devmath::logf_(v3))));
                float n2 = nd.draw(src, 0.0f, 1.0f);
                float vb = 1.0f + a2 * n2;
                float vb3 = vb * vb * vb;
                float ub = hml_canonical_f32(src);
                const bool d1 = (double)ub > (double)1.0f - 0.0331 * (double)n2 * (double)n2 * (double)n2 * (double)n2;
                const bool d2 = ((double)hml_devmath::logf_(ub) > (0.5 * (double)n2 * (double)n2 + (double)a1 * ((1.0 - (double)vb3) + (double)hml_devmath::logf_(vb3))));
                r = fn == 12 ? n : fn == 13 ? v3 : fn == 14 ? u : fn == 15 ? (float)(c1 ? 1 : 0) + 2.0f * (c2 ? 1 : 0) : fn == 16 ? n2 : fn == 17 ? a2
                    : fn == 18 ? vb3 : fn == 19 ? ub : fn == 20 ? (float)(d1 ? 1 : 0) + 2.0f * (d2 ? 1 : 0) : fn == 21 ? (float)src.s.n : 0.0f;
                if (fn == 22) r = nd.draw(src, 0.0f, 1.0f);   // third normal (fresh pair)
                if (fn == 23) { hml_normal_f32<hml_devmath> nf; r = nf.draw(src, 0.0f, 1.0f); r = nf.draw(src, 0.0f, 1.0f); }  // saved of the fresh pair
            } break;
            case 30: case 31: {   // categorical draw over K = 16 / 5 weights a[i..i+K), u = b[i]: out = {combined, literal, unsure}
                r = 0.0f;
                const int Kc = fn == 30 ? 16 : 5;
                if (i % Kc == 0 && i + Kc <= n) {
                    bool unsure = false;
                    int fastr, lit;
                    if (fn == 30) { float w[16]; for (int j = 0; j < 16; ++j) w[j] = a[i + j]; fastr = hml_categorical_k_fast<16>(w, (double)y, unsure); lit = hml_categorical_k_literal<16>(w, (double)y); if (unsure) fastr = lit; }
                    else { float w[5]; for (int j = 0; j < 5; ++j) w[j] = a[i + j]; fastr = hml_categorical_k_fast<5>(w, (double)y, unsure); lit = hml_categorical_k_literal<5>(w, (double)y); if (unsure) fastr = lit; }
                    out[i] = (float)fastr; out[i + 1] = (float)lit; out[i + 2] = unsure ? 1.0f : 0.0f;
                }
                continue;
            }
            case 11: { const double d = HML_SQRT((double)x * 1.0000001); r = (float)((d - (double)(float)d) * 1e9); } break;
        }
        out[i] = r;
    }
}

// ---- the edges of the level bands (hml_set_level_bands; HML_BANDS=e0,e1,... for unmodified callers)
static bool parse_band_edges(const char* text, int* n, float* edges) {
    // "e0,e1,..." (HML_BANDS); false on anything else
    *n = 0;
    const char* p = text;
    while (*p) {
        char* end = nullptr;
        const float v = strtof(p, &end);
        if (end == p || *n >= HML_MAX_BAND_EDGES) return false;
        edges[(*n)++] = v;
        p = end;
        if (*p == ',') ++p; else if (*p) return false;
    }
    return *n > 0;
}

static const char* band_edges_fault(int n, const float* edges) {
    if (n < 1 || n > HML_MAX_BAND_EDGES) return "level bands take 1 to 31 edges";
    for (int j = 0; j < n; ++j) {
        if (!std::isfinite(edges[j])) return "the edges of the level bands must be finite";
        if (j > 0 && !(edges[j - 1] < edges[j])) return "the edges of the level bands must be strictly ascending";
    }
    return nullptr;
}

static int bands_from_env(hml_ctx* c) {
    if (const char* e = getenv("HML_BANDS")) {
        int n = 0; float edges[HML_MAX_BAND_EDGES];
        if (!parse_band_edges(e, &n, edges)) return set_err(HML_ERR_ARG, "HML_BANDS: expected up to 31 comma-separated numbers");
        if (const char* why = band_edges_fault(n, edges)) return set_err(HML_ERR_ARG, std::string("HML_BANDS: ") + why);
        c->n_band_edges = n;
        memcpy(c->band_edges, edges, (size_t)n * sizeof(float));
        c->rec[HML_REC_BANDS].on = c->rec[HML_REC_BANDS].asked = true;
    }
    return 0;
}

extern "C" {

const char* hml_last_error(void) { return g_err.c_str(); }
uint32_t hml_abi_version(void) { return 5; }   // 2: hml_stats.fused_fallbacks, hml_allreduce_marginals_perm, hml_pool_permutation, option "compat"; 3: hml_attach_observations;
                                                // 4: emission levels per position (hml_set_level_recording, hml_levels_rle, hml_levels_dense_device, hml_levels_merge)
                                                // 5: breakpoint posteriors (hml_set_break_recording, hml_breaks_list, hml_breaks_dense_device, hml_breaks_merge,
                                                //    hml_breaks_consensus) and hml_levels_on_segments
const char* hml_device_arch(void) { return "gfx950"; }
int hml_device_count(int* n) {
    if (!n) return set_err(HML_ERR_ARG, "null argument");
    HIPCHK(hipGetDeviceCount(n));
    return 0;
}

// the context goes, and with it every buffer it owns; its own stream last
static void delete_ctx(hml_ctx* c) {
    const hipStream_t own = c->own_stream ? c->stream : nullptr;
    delete c;
    if (own) hipStreamDestroy(own);
}

// allocations of a fresh context; on failure the caller deletes it
static int create_inner(hml_ctx* c, void* stream) {
    HIPCHK(hipSetDevice(c->device));
    if (stream) { c->stream = (hipStream_t)stream; c->own_stream = false; }
    else { HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)); c->own_stream = true; }
    HIPCHK(c->d_mdl.alloc(1));
    HIPCHK(hipMemsetAsync(c->d_mdl, 0, sizeof(hml_model), c->stream));
    HIPCHK(hipHostMalloc(&c->h_B, 4 * sizeof(uint32_t), hipHostMallocMapped));
    c->h_B[0] = 0; c->h_B[1] = 0; c->h_B[2] = 0; c->h_B[3] = 0;
    void* d_hB = nullptr;
    HIPCHK(hipHostGetDevicePointer(&d_hB, c->h_B, 0));
    c->d_hB = static_cast<uint32_t*>(d_hB);
    return 0;
}

// a chunk length from the environment: the largest power of two up to the value, of at most `max_bits` bits
static void env_chunk_length(const char* name, int max_bits, int* L) {
    if (const char* e = getenv(name)) { const int l = std::max(1, atoi(e)); int sh = 0; while ((1 << (sh + 1)) <= l && sh < max_bits) ++sh; *L = 1 << sh; }
}

int hml_create(hml_ctx** out, int device, uint64_t seed, uint32_t chain_id, void* stream) {
    if (!out) return set_err(HML_ERR_ARG, "null output pointer");
    int n = 0;
    HIPCHK(hipGetDeviceCount(&n));
    if (n <= 0) return set_err(HML_ERR_HIP, "no HIP device available: the MI355X kernels cannot run (there is no CPU fallback)");
    if (device < 0 || device >= n) return set_err(HML_ERR_ARG, "device index out of range");
    hml_ctx* c = new hml_ctx();
    c->device = device; c->seed = seed; c->chain = chain_id;
    if (int r = create_inner(c, stream)) { delete_ctx(c); return r; }
    hml_sweep_knobs& kn = c->knobs;
    env_chunk_length("HML_FWD_CHUNK", 10, &kn.geo[HML_GEO_SPARSE].L);
    if (const char* e = getenv("HML_FWD_WARMUP")) c->fwdW = c->fwdW_init = std::max(0, atoi(e));
    if (const char* e = getenv("HML_FWD_BURNIN_SWEEPS")) c->fwd_burnin_sweeps = (uint32_t)std::max(0, atoi(e));
    if (const char* e = getenv("HML_FWD_QUIET")) c->fwd_quiet_need = (uint32_t)std::max(1, atoi(e));
    env_chunk_length("HML_FWD_CHUNK_MANY", 6, &kn.geo[HML_GEO_MANY].L);
    env_chunk_length("HML_FWD_CHUNK_MID", 10, &kn.geo[HML_GEO_MID].L);
    if (const char* e = getenv("HML_MID_MIN_BLOCKS")) kn.mid_min_blocks = (uint32_t)strtoul(e, nullptr, 10);
    env_chunk_length("HML_FWD_CHUNK_DENSE", 10, &kn.geo[HML_GEO_DENSE].L);
    if (const char* e = getenv("HML_DENSE_MIN_BLOCKS")) kn.dense_min_blocks = (uint32_t)strtoul(e, nullptr, 10);
    if (const char* e = getenv("HML_USE_GRAPH")) c->use_graph = atoi(e) != 0;
    if (const char* e = getenv("HML_WEIGHT_KEYS")) kn.use_keys = atoi(e) != 0;
    if (const char* e = getenv("HML_FUSED_BLOCKS")) { kn.fused_blocks = atoi(e) != 0; kn.fused_keep = atoi(e) == 2; }   // 0: a GPU shared with other processes
    if (const char* e = getenv("HML_TRELLIS_FUSED")) kn.tre_fused = atoi(e) != 0;
    if (const char* e = getenv("HML_TRELLIS_L")) { const int l = atoi(e); c->tre_L = (l <= 0) ? 0u : (l >= HML_TRE_MAX_L) ? (uint32_t)HML_TRE_MAX_L : (l < 32) ? 32u : (uint32_t)l / 32u * 32u; }   // a multiple of 32
    if (const char* e = getenv("HML_TRELLIS_CKPT")) c->tre_ckpt = atoi(e) != 0;
    if (const char* e = getenv("HML_TRELLIS_REFIT_ROUNDS")) { const int r = atoi(e); c->tre_refit_rounds = r < 0 ? 0u : r > 6 ? 6u : (uint32_t)r; }
    if (const char* e = getenv("HML_STAGE_BITS")) kn.stage_bits = atoi(e) != 0;
    if (const char* e = getenv("HML_TRELLIS_ROWS")) kn.tre_rows = atoi(e) != 0;   // 0: round 2's first pass (hml_k_trellis_tile) for comparison
    if (const char* e = getenv("HML_LATE_RESCALE")) kn.late_rescale = atoi(e) != 0;
    if (const char* e = getenv("HML_PARAMS_SPREAD")) kn.params_spread = atoi(e) != 0;
    if (const char* e = getenv("HML_COMPAT_CHUNKS")) c->rtk.compat_chunks = atoi(e);   // (1: the sequential form; > 1: that many chunks)
    if (const char* e = getenv("HML_COMPAT_WARMUP")) c->rtk.compat_warmup = atoi(e);   // (tests: a warm-up too short to forget the start)
    if (const char* e = getenv("HML_WIDE_LANES")) c->rtk.wide_lanes = atoi(e);   // (0: models of more than 16 states with a state a lane)
    if (const char* e = getenv("HML_WIDE_W0")) c->rtk.wide_w0 = std::max(8, atoi(e));
    if (const char* e = getenv("HML_WIDE_MAX_CHUNKS")) c->rtk.wide_max_chunks = (uint32_t)std::max(64, atoi(e));
    if (const char* e = getenv("HML_WIDE_L")) {   // (tests: chunks of that many blocks, a power of two)
        const int L = atoi(e);
        if (L >= 1) { int sh = 0; while ((1 << sh) < L && sh < 20) ++sh; c->rtk.wide_lshift = sh; }
    }
    if (const char* e = getenv("HML_COMPAT")) c->compat = atoi(e) != 0;   // option "compat" for unmodified callers (`hammlet -compat`)
    if (const char* e = getenv("HML_TRELLIS_TUNE")) c->tre_autotune = atoi(e) != 0;
    if (const char* e = getenv("HML_FUSED_SPIN_LIMIT")) c->fused_spin_limit = (uint32_t)strtoul(e, nullptr, 10);
    if (const char* e = getenv("HML_LEVELS")) c->rec[HML_REC_LEVELS].on = c->rec[HML_REC_LEVELS].asked = atoi(e) != 0;   // hml_set_level_recording for unmodified callers (`hammlet -O L`)
    if (const char* e = getenv("HML_BREAKS")) c->rec[HML_REC_BREAKS].on = c->rec[HML_REC_BREAKS].asked = atoi(e) != 0;   // hml_set_break_recording for unmodified callers (`hammlet -O breakpoints`)
    if (const char* e = getenv("HML_MAX_BLOCKS")) c->cap_opt = strtoull(e, nullptr, 10);   // option "max_blocks" (tests: a tiny capacity exercises the growth everywhere)
    if (device < 64) g_live_ctx[device].fetch_add(1);
    if (int r = bands_from_env(c)) { hml_destroy(c); return r; }   // HML_BANDS=e0,e1,...: hml_set_level_bands for unmodified callers (`hammlet -bands`)
    *out = c;
    return 0;
}

// the shared construction this context reads (none: nullptr), and the context's views of it; the last context that holds a
// construction frees it
static void set_trace(hml_ctx* c, std::shared_ptr<hml_trace> tr) {
    c->trace = std::move(tr);
    const hml_trace* t = c->trace.get();
    c->d_w = t ? t->d_w.get() : nullptr; c->d_summary = t ? t->d_summary.get() : nullptr;
    c->d_coeff = t ? t->d_coeff.get() : nullptr; c->d_ia = t ? t->d_ia.get() : nullptr;
}
static bool trace_shared(const hml_ctx* c) { return c->trace.use_count() > 1; }

void hml_destroy(hml_ctx* c) {
    if (!c) return;
    if (c->device < 64) g_live_ctx[c->device].fetch_sub(1);
    hipSetDevice(c->device);
    hipStreamSynchronize(c->stream);
    for (auto& kv : c->prof) for (auto& p : kv.second.pending) { hipEventDestroy(p.first); hipEventDestroy(p.second); }
    for (auto e : c->ev_pool) hipEventDestroy(e);
    drop_graph(c);
    delete_ctx(c);
}

// ---------------------------------------------------------------------------------------- load
// 8-bit keys of the current weights, bucket window centred on the universal threshold of the noise estimate
static int build_keys(hml_ctx* c) {
    if (!c->knobs.use_keys) return 0;
    const uint64_t T = c->T;
    if (!c->d_summary) {
        // one byte per 16-position group, padded with zeros to whole spans
        const uint64_t n_spans = (T + HML_SPAN - 1) / HML_SPAN;
        HIPCHK(c->trace->d_summary.alloc(n_spans * (HML_SPAN / 16) + 16));
        c->d_summary = c->trace->d_summary;
        HIPCHK(hipMemsetAsync(c->d_summary, 0, n_spans * (HML_SPAN / 16) + 16, c->stream));
    }
    const float thr0 = (float)(std::sqrt(2 * std::log((double)std::max<uint64_t>(T, 2))) * c->sigma * c->key_scale);
    uint32_t u; memcpy(&u, &thr0, 4);
    c->key_base = (std::isfinite(thr0) && thr0 > 0 ? (int32_t)(u >> 20) : (int32_t)(0x3f800000u >> 20)) - 128;
    hipLaunchKernelGGL(hml_k_build_summary, dim3(grid_for((T + 15) / 16, 256, 1, 65536)), dim3(256), 0, c->stream, c->d_w, T,
                       c->key_base, c->d_summary);
    KLAUNCH_CHECK();
    return 0;
}

HML_KERNEL void hml_k_max_inplace(float* __restrict__ a, const float* __restrict__ b, uint64_t n) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) { const float x = a[i], y = b[i]; a[i] = (x < y) ? y : x; }   // std::max(x, y)
}

enum { CAPBUF_BLOCKS = 1, CAPBUF_PROBES = 2, CAPBUF_SWEEP = 4 };
static int alloc_capacity_buffers(hml_ctx* c, int what);   // (below)

// the per-chain block-structure buffers (every context has its own; the construction above them may be shared)
static int alloc_block_buffers(hml_ctx* c) {
    const uint64_t T = c->T;
    c->n_spans = (uint32_t)((T + HML_SPAN - 1) / HML_SPAN);
    HIPCHK(c->d_stage.alloc((uint64_t)c->n_spans * HML_SPAN));
    HIPCHK(c->d_span_count.alloc(c->n_spans));
    HIPCHK(c->d_coarse1.alloc((c->n_spans + HML_GROUP_SPANS - 1) / HML_GROUP_SPANS + 1u));
    {
        const uint64_t n_tiles = (T + HML_FUSED_SUB_POSITIONS - 1) / HML_FUSED_SUB_POSITIONS;   // (tiles of one batch: the most there can be)
        HIPCHK(c->d_group_word.alloc(n_tiles + 1));
        HIPCHK(hipMemsetAsync(c->d_group_word, 0, (n_tiles + 1) * sizeof(unsigned long long), c->stream));
        HIPCHK(c->d_wave_total.DevBuf::alloc(hml_layout_wave_total(nullptr, n_tiles).bytes));
        if (getenv("HML_FUSED_DEBUG")) { HIPCHK(c->d_dbg.alloc(4096 * 8)); HIPCHK(hipMemset(c->d_dbg, 0, 4096 * 8 * 8)); }
    }
    if (int r = alloc_capacity_buffers(c, CAPBUF_BLOCKS)) return r;
    // the capacity the enumeration kernels respect (they run before there is a model: auto prior, explicit thresholds)
    const uint32_t cap32 = (uint32_t)c->cap;
    HIPCHK(hipMemcpyAsync(&c->d_mdl->cap, &cap32, sizeof cap32, hipMemcpyHostToDevice, c->stream));
    return 0;
}

// the block capacity of a context whose observations are being loaded (`attached`: to another context's construction)
static void choose_capacity(hml_ctx* c, bool attached) {
    const uint64_t T = c->T;
    uint64_t cap = T;
    if (c->D == 1) {
        if (c->cap_opt) cap = c->cap_opt;
        // a further chain on a GPU (hml_attach_observations): room for the strongly compressed regime (up to 2^22 blocks a sweep,
        // or a sixteenth of the positions) instead of the worst case - it grows if a sweep needs more
        else if (attached) cap = std::max<uint64_t>(1ull << 20, T / 16);
    }
    c->cap = std::min<uint64_t>(std::max<uint64_t>(cap, 64), T);
}

// d_x[d], h_x[d]: the observations of dimension d (T values each), on the device and on the host
static int build_from_device_x(hml_ctx* c, const float* const* d_x, const float* const* h_x) {
    const uint64_t T = c->T;
    const int D = c->D;
    set_trace(c, std::make_shared<hml_trace>());   // (an earlier load that failed half-way: its construction goes first)
    // noise estimate (src/main.cpp:303-311): f64 accumulation, in index order, of the finest-level
    // maxlet coefficients c[t] = max over the dimensions of sqrt2half * |x[t-1] - x[t]| at odd t
    // (wavelet.hpp:139-158, level 1)
    {
        const float sqrt2 = (float)std::sqrt(2.0);
        const float sqrt2half = (float)(sqrt2 / 2.0);
        double acc = 0; uint64_t cnt = 0;
        for (uint64_t i = 1; i < T; i += 2) {
            float mx = 0.0f;
            for (int d = 0; d < D; ++d) {
                const float df = std::abs(h_x[d][i - 1] - h_x[d][i]);
                const float cf = sqrt2half * df;
                mx = (mx < cf) ? cf : mx;
            }
            acc += mx;
            cnt++;
        }
        acc /= cnt;
        acc /= 0.797884560802865355879892119868763736951717262329869315331;
        c->sigma = acc;
    }
    HIPCHK(c->trace->d_w.alloc(T));
    HIPCHK(c->trace->d_coeff.alloc(T));
    HIPCHK(c->trace->d_ia.alloc((T + 1) * (uint64_t)D));
    set_trace(c, c->trace);
    // K1: levels 10 at a time, one dimension after the other; the coefficient is the maximum over the dimensions
    {
        float h_norm[64];
        const float sqrt2 = (float)std::sqrt(2.0);
        const float sqrt2half = (float)(sqrt2 / 2.0);
        h_norm[0] = 1.0f;
        float nrm = sqrt2half;
        for (int l = 1; l < 64; ++l) { h_norm[l] = nrm; nrm *= sqrt2half; }
        DevArr<float> s_norm, s_a, s_b, s_other;   // freed on every path out of this scope
        HIPCHK(s_norm.alloc(64));
        float* d_norm = s_norm;
        HIPCHK(hipMemcpyAsync(d_norm, h_norm, sizeof h_norm, hipMemcpyHostToDevice, c->stream));
        const uint64_t n1 = T >> HML_MAXLET_LOG_TILE;
        HIPCHK(s_a.alloc(std::max<uint64_t>(n1, 1)));
        HIPCHK(s_b.alloc(std::max<uint64_t>(n1 >> HML_MAXLET_LOG_TILE, 1)));
        if (D > 1) HIPCHK(s_other.alloc(T));
        float *bufA = s_a, *bufB = s_b, *d_other = s_other;
        for (int d = 0; d < D; ++d) {
            float* coeff_out = d == 0 ? c->d_coeff : d_other;
            uint64_t n = T;
            int base = 0;
            const float* in = d_x[d];
            float* outb = bufA;
            while (true) {
                const uint64_t tiles = (n + HML_MAXLET_TILE - 1) / HML_MAXLET_TILE;
                hipLaunchKernelGGL(hml_k_maxlet, dim3((unsigned)tiles), dim3(256), 0, c->stream, in, n, base, coeff_out, T, outb, d_norm);
                KLAUNCH_CHECK();
                base += HML_MAXLET_LOG_TILE;
                if (base >= 40 || (1ull << base) >= T) break;   // no discontinuity position left below T
                n = T >> base;                                   // complete elements of the next level (>= 1)
                in = outb;
                outb = (outb == bufA) ? bufB : bufA;
            }
            if (d > 0) {
                hipLaunchKernelGGL(hml_k_max_inplace, dim3(grid_for(T, 256, 1, 65536)), dim3(256), 0, c->stream, c->d_coeff, d_other, T);
                KLAUNCH_CHECK();
            }
        }
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    hipLaunchKernelGGL(hml_k_weights, dim3(grid_for(T, 256, 1, 65536)), dim3(256), 0, c->stream, c->d_coeff, c->d_w, T, 1.0f);
    KLAUNCH_CHECK();
    if (int r = build_keys(c)) return r;
    {
        const uint64_t cells = (T + 1 + HML_CELLSIZE - 1) / HML_CELLSIZE;
        for (int d = 0; d < D; ++d) {
            hipLaunchKernelGGL(hml_k_integral, dim3((unsigned)((cells + 3) / 4)), dim3(256), 0, c->stream, d_x[d], c->d_ia + (uint64_t)d * (T + 1), T);
            KLAUNCH_CHECK();
        }
    }
    choose_capacity(c, false);
    if (int r = alloc_block_buffers(c)) return r;
    HIPCHK(hipStreamSynchronize(c->stream));
    c->loaded = true;
    return 0;
}

// "-s C P D" (reference src/main.cpp:114-137, src/Mapping.hpp:53-137): D data dimensions whose values follow each other
// in the observation stream, P emission parameters shared by the K = P^D states.  Before the observations are loaded.
int hml_set_dimensions(hml_ctx* c, int D, int P) {
    if (!c) return set_err(HML_ERR_ARG, "null context");
    if (c->loaded) return set_err(HML_ERR_ARG, "dimensions must be set before the observations are loaded");
    if (D <= 0) return set_err(HML_ERR_MODEL, "Number of data dimensions must be positive!");
    if (P < 0) return set_err(HML_ERR_MODEL, "Number of parameters must be positive!");
    if (D > HML_MAX_D) return set_err(HML_ERR_ARG, "at most 4 data dimensions are supported");
    if (P > 0) {   // P = 0: taken from hml_set_model's number of states (K = P^D)
        long k = 1;
        for (int d = 0; d < D; ++d) { k *= P; if (k > HML_CAP_K) return set_err(HML_ERR_ARG, "number of states must be in [2,64]"); }
        if (k <= 1) return set_err(HML_ERR_MODEL, "Requested parameters would yield an HMM with less than 2 states!");
    }
    c->D = D; c->P = P;
    return 0;
}

// x: T * D values, the D dimensions of a position one after the other (T values when D = 1)
int hml_load_observations(hml_ctx* c, const float* x, uint64_t n_values) {
    if (!c || !x) return set_err(HML_ERR_ARG, "null argument");
    if (n_values == 0) return set_err(HML_ERR_ARG, "Input vector for breakpoint weights is empty!");
    const uint64_t D = (uint64_t)c->D;
    if (n_values % D != 0) return set_err(HML_ERR_MODEL, "Input stream did not contain enough values to fill all dimensions at last position!");
    const uint64_t T = n_values / D;
    if (T >= 0xffffffffull) return set_err(HML_ERR_ARG, "at most 2^32-2 positions are supported");
    if (c->loaded) return set_err(HML_ERR_ARG, "observations already loaded");
    if (int r = ctx_bind(c)) return r;
    c->T = T;
    DevArr<float> s_x;
    HIPCHK(s_x.alloc(n_values));
    float* d_x = s_x;
    std::vector<float> planes;             // dimension-major copy when D > 1
    const float* h_dim[HML_MAX_D];
    const float* d_dim[HML_MAX_D];
    if (D == 1) { h_dim[0] = x; }
    else {
        planes.resize(n_values);
        for (uint64_t t = 0; t < T; ++t) for (uint64_t d = 0; d < D; ++d) planes[d * T + t] = x[t * D + d];
        for (uint64_t d = 0; d < D; ++d) h_dim[d] = planes.data() + d * T;
    }
    HIPCHK(hipMemcpyAsync(d_x, D == 1 ? x : planes.data(), n_values * sizeof(float), hipMemcpyHostToDevice, c->stream));
    for (uint64_t d = 0; d < D; ++d) d_dim[d] = d_x + d * T;
    return build_from_device_x(c, d_dim, h_dim);
}

int hml_load_observations_device(hml_ctx* c, const void* x_dev, uint64_t T) {
    if (!c || !x_dev) return set_err(HML_ERR_ARG, "null argument");
    if (c->D != 1) return set_err(HML_ERR_ARG, "device input is univariate");
    if (T == 0) return set_err(HML_ERR_ARG, "Input vector for breakpoint weights is empty!");
    if (T >= 0xffffffffull) return set_err(HML_ERR_ARG, "at most 2^32-2 positions are supported");
    if (c->loaded) return set_err(HML_ERR_ARG, "observations already loaded");
    if (int r = ctx_bind(c)) return r;
    c->T = T;
    std::vector<float> h(T);
    HIPCHK(hipMemcpy(h.data(), x_dev, T * sizeof(float), hipMemcpyDeviceToHost));
    const float* h_dim[1] = {h.data()};
    const float* d_dim[1] = {(const float*)x_dev};
    return build_from_device_x(c, d_dim, h_dim);
}

// A second chain over the SAME observations on the same device: shares the source's read-only construction (weights,
// summary, coefficients, integral arrays - reference counted) instead of building a private copy; block structure and sweep
// buffers stay per chain.  The reference holds one chain per process over its one trace (src/main.cpp:108,338-343).
int hml_attach_observations(hml_ctx* c, hml_ctx* src) {
    if (!c || !src) return set_err(HML_ERR_ARG, "null argument");
    if (c == src) return set_err(HML_ERR_ARG, "a context cannot be attached to itself");
    if (!src->loaded || !src->trace) return set_err(HML_ERR_ARG, "the source context has no observations loaded");
    if (c->loaded) return set_err(HML_ERR_ARG, "observations already loaded");
    if (c->device != src->device) return set_err(HML_ERR_ARG, "contexts that share observations must live on one device");
    if (c->knobs.use_keys != src->knobs.use_keys) return set_err(HML_ERR_ARG, "option weight_keys differs from the source context's");
    if (int r = ctx_bind(c)) return r;
    HIPCHK(hipStreamSynchronize(src->stream));   // (a weight multiplier still on its way)
    c->T = src->T; c->D = src->D;
    if (c->P == 0 || c->D > 1) c->P = src->P;
    c->sigma = src->sigma; c->key_base = src->key_base; c->key_scale = src->key_scale;
    set_trace(c, src->trace);
    choose_capacity(c, true);
    if (int r = alloc_block_buffers(c)) { set_trace(c, nullptr); return r; }
    HIPCHK(hipStreamSynchronize(c->stream));
    c->loaded = true;
    return 0;
}

int hml_noise_sigma(hml_ctx* c, double* sigma) {
    if (!c || !c->loaded) return set_err(HML_ERR_ARG, "no observations loaded");
    *sigma = c->sigma;
    return 0;
}

int hml_scale_weights(hml_ctx* c, float mult) {
    if (!c || !c->loaded) return set_err(HML_ERR_ARG, "no observations loaded");
    if (trace_shared(c)) return set_err(HML_ERR_ARG, "the weights are shared with attached contexts: scale them before hml_attach_observations");
    if (int r = ctx_bind(c)) return r;
    hipLaunchKernelGGL(hml_k_scale, dim3(grid_for(c->T, 256, 1, 65536)), dim3(256), 0, c->stream, c->d_w, c->T, mult);
    KLAUNCH_CHECK();
    c->key_scale *= std::fabs((double)mult) > 0 ? std::fabs((double)mult) : 1.0;
    if (int r = build_keys(c)) return r;
    c->blocks_valid = false;
    return 0;
}

int hml_set_weights(hml_ctx* c, const float* w, uint64_t T) {
    if (!c || !c->loaded || !w) return set_err(HML_ERR_ARG, "no observations loaded");
    if (T != c->T) return set_err(HML_ERR_MODEL, "Block structure and statistics have different number of data points!");
    if (trace_shared(c)) return set_err(HML_ERR_ARG, "the weights are shared with attached contexts: set them before hml_attach_observations");
    if (int r = ctx_bind(c)) return r;
    HIPCHK(hipMemcpyAsync(c->d_w, w, T * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    // the key window stays centred on the noise estimate times the multipliers applied through hml_scale_weights: the
    // window only decides how many groups the summary scan opens, never which positions start a block
    if (int r = build_keys(c)) return r;
    c->blocks_valid = false;
    c->hint_stale = true;
    return 0;
}

}  // extern "C"

static int grow_capacity(hml_ctx* c, uint64_t needed);
// an enumeration at an explicit threshold (with block statistics), waited for; a context with a reduced block capacity
// grows until the blocks fit (hml_state.h)
static int enumerate_blocks_sync(hml_ctx* c, float threshold) {
    if (int r = settle_if_limited(c)) return r;   // (sweeps still under way come first)
    for (int round = 0; round < 64; ++round) {
        if (int r = launch_compact(c, true, threshold)) return r;
        HIPCHK(hipStreamSynchronize(c->stream));
        if (!chain_halted(c)) return 0;
        if (int r = grow_capacity(c, c->h_B[2])) return r;
    }
    return set_err(HML_ERR_HIP, "internal error: the block capacity did not settle");
}
extern "C" {

int hml_create_blocks(hml_ctx* c, float threshold) {
    if (!c || !c->loaded) return set_err(HML_ERR_ARG, "no observations loaded");
    if (int r = ctx_bind(c)) return r;
    if (int r = enumerate_blocks_sync(c, threshold)) return r;
    refresh_hint(c);
    c->blocks_valid = false;   // an explicit threshold is not the model's threshold
    return 0;
}

int hml_autoprior(hml_ctx* c, float s2, float p, float out4[4]) {
    if (!c || !c->loaded) return set_err(HML_ERR_ARG, "no observations loaded");
    if (int r = ctx_bind(c)) return r;
    // y.createBlocks( sqrt(2*log((double)T)) * noiseStdev )   (AutoPriors.hpp:95-96)
    const float thr0 = (float)(std::sqrt(2 * std::log((double)c->T)) * c->sigma);
    if (int r = enumerate_blocks_sync(c, thr0)) return r;
    refresh_hint(c);
    const uint32_t B = *c->h_B;
    std::vector<uint32_t> st(B + 1);
    const int D = c->D;
    std::vector<float2> bs((size_t)B * D);
    HIPCHK(hipMemcpy(st.data(), c->d_starts, (B + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (int d = 0; d < D; ++d)
        HIPCHK(hipMemcpy(bs.data() + (size_t)d * B, c->d_bstat + (uint64_t)d * c->cap, B * sizeof(float2), hipMemcpyDeviceToHost));   // (D > 1: cap = T)
    // block means in block order, every dimension of a block in turn (AutoPriors.hpp:100-104), float accumulation
    // (SufficientStatistics<Normal>::addObs); N = nrBlocks * nrDim (AutoPriors.hpp:105)
    float muSum = 0, muSq = 0;
    for (uint32_t b = 0; b < B; ++b) {
        for (int d = 0; d < D; ++d) {
            const float m = bs[(size_t)d * B + b].x / (float)(st[b + 1] - st[b]);
            muSum += m;
            muSq += m * m;
        }
    }
    const double n = (double)((uint64_t)B * (uint64_t)D);
    const double blocksMean = (double)(float)(muSum / n);
    const double avg = (double)(float)(muSum / n);
    const double blocksVar = (double)(float)(muSq / n - (avg * avg));
    const float dataMean = (float)blocksMean, dataVar = (float)blocksVar;
    if (p < 0 || p > 1) return set_err(HML_ERR_MODEL, "Parameter p for automatic priors is a probability and must be in [0,1]!");
    if (s2 <= 0) return set_err(HML_ERR_MODEL, "Parameter s2  for automatic priors is a variance and must be positive!");
    if (dataVar <= 0) return set_err(HML_ERR_MODEL, "Data variance provided to autoprior must be positive!");
    const float M1 = 0.3361, M2 = -0.0042, M3 = -0.0201;
    const float b = -std::log(p);
    const float alpha = 2.0;
    const float beta = s2 * ((2.0 * std::sqrt(b)) / (M1 * std::sqrt(b) + std::sqrt(2.0) * (M2 * b * std::exp(M3 * std::sqrt(b)) + 1)) + b);
    const float mu0 = dataMean;
    const float nu = beta / dataVar;
    if (beta <= 0) return set_err(HML_ERR_MODEL, "Autoprior yields non-positive beta!");
    if (nu <= 0) return set_err(HML_ERR_MODEL, "Autoprior yields non-positive nu!");
    if (!std::isfinite(beta)) return set_err(HML_ERR_MODEL, "Autoprior yields non-finite beta!");
    if (!std::isfinite(mu0)) return set_err(HML_ERR_MODEL, "Autoprior yields non-finite mu0!");
    if (!std::isfinite(nu)) return set_err(HML_ERR_MODEL, "Autoprior yields non-finite nu!");
    out4[0] = alpha; out4[1] = beta; out4[2] = mu0; out4[3] = nu;
    return 0;
}

}  // extern "C"

// the per-block sweep buffers of the default path, sized by the context's block capacity (hml_ctx.hpp; c->K set)
int hml_alloc_sweep_default(hml_ctx* c) {
    const int K = c->K;
    const uint64_t cap = c->cap;
    int minL = c->knobs.geo[0].L;
    for (const hml_fwd_geo& g : c->knobs.geo) minL = std::min(minL, g.L);
    const uint64_t maxChunks = (cap + minL - 1) / minL + 1;   // per-chunk arrays serve either geometry
    uint64_t plane = 0;   // floats in one chunk-transposed [L][K][cstride] array
    auto layout = [&](int L, hml_layout& lay) {
        int sh = 0; while ((1 << sh) < L) ++sh;
        lay.lshift = (uint32_t)sh;
        lay.cstride = (uint32_t)(((cap + L - 1) / L + 1 + 63) / 64 * 64);
        plane = std::max(plane, (uint64_t)L * K * lay.cstride);
    };
    for (hml_fwd_geo& g : c->knobs.geo) layout(g.L, g.lay);
    HIPCHK(c->d_em.alloc(plane));
    HIPCHK(c->d_gsc.alloc(plane));
    HIPCHK(c->d_rows.alloc(plane));
    HIPCHK(c->d_entry.alloc(maxChunks * K));
    HIPCHK(c->d_exitA.alloc(maxChunks * K));
    HIPCHK(c->d_fb.alloc(maxChunks));
    HIPCHK(c->d_smap.alloc(cap + 2));
    // per-chunk arrays serve the backward chunks of 64 rows and the fused trellis path's forward chunks of 16 or 32
    const uint64_t bchunks = (cap + 15) / 16 + 1;
    HIPCHK(c->d_cmap.alloc(bchunks));
    HIPCHK(c->d_bentry.alloc(bchunks));
    HIPCHK(c->d_scmap.alloc(bchunks));
    HIPCHK(c->d_super.alloc(bchunks / 64 + 2));
    HIPCHK(c->d_bentry2.alloc(bchunks / 64 + 2));
    HIPCHK(c->d_redo.alloc(bchunks));
    HIPCHK(hipMemsetAsync(c->d_redo, 0, bchunks * sizeof(uint32_t), c->stream));
    HIPCHK(c->d_touched.alloc(bchunks));
    HIPCHK(hipMemsetAsync(c->d_touched, 0, bchunks * sizeof(uint32_t), c->stream));
    HIPCHK(c->d_redo2.alloc(bchunks));
    HIPCHK(c->d_tre_bitmap.alloc(bchunks / 32 + 2));
    // (checkpoints of the fused trellis path: (L / 64 - 1) x ceil(B / L) <= B / 64 + 16 vectors of K + 1 words)
    HIPCHK(c->d_tre_ckpt.alloc((cap / HML_TRE_CKPT_ROWS + 64) * (uint64_t)(K + 1)));
    HIPCHK(c->d_q.alloc(cap));
    // (the count pass's group partials [2 K][1024] and, behind them, the first level of their tree [16][2 K]: hml_k_params.h)
    const uint64_t n_partial = ((uint64_t)HML_REDUCE_GROUPS + HML_PARAMS_TREE_WGS) * K * 2;
    HIPCHK(c->d_partial.alloc(n_partial));
    HIPCHK(hipMemsetAsync(c->d_partial, 0, n_partial * sizeof(double), c->stream));
    return 0;
}

// Everything that is sized by the block capacity, in ONE place: block starts and statistics (from the load on), the probes
// (hml_enable_probes) and the sweep buffers (from the model on).  Allocating a buffer replaces what it held, so a call that
// failed half-way is simply made again.
static int alloc_capacity_buffers(hml_ctx* c, int what) {
    if (what & CAPBUF_BLOCKS) {
        HIPCHK(c->d_starts.alloc(c->cap + 1));
        HIPCHK(c->d_bstat.alloc(c->cap * (uint64_t)c->D));   // (D > 1: cap = T, the planes lie T apart)
    }
    if (what & CAPBUF_PROBES) {
        HIPCHK(c->d_eprobe.alloc(c->cap * c->K));
        HIPCHK(c->d_aprobe.alloc((c->cap + 1) * c->K));
    }
    return (what & CAPBUF_SWEEP) ? c->kt->alloc_sweep(c) : 0;   // (of the context's path: hml_ktab)
}

// More room for blocks: the per-block buffers are allocated again for at least `needed` blocks (half as many again, at least
// twice the old capacity, at most T).  Nothing in them outlives a sweep except a static block structure, which the next sweep
// enumerates again; the reference-compatible mode's engine (d_mt) is not among them and lives on.  Buffer by buffer: every
// new one is at least as large as the one it replaces, so the device never holds more than the new total.  The stream is idle.
// A failure leaves the capacity as it was and the chain halted: the next entry point comes here again (hml_settle) before
// anything is launched.
static int grow_capacity(hml_ctx* c, uint64_t needed) {
    const uint64_t old_cap = c->cap;
    drop_graph(c);
    c->cap = std::min<uint64_t>(c->T, std::max<uint64_t>(needed + needed / 2 + 1024, 2 * old_cap));
    const uint32_t words[2] = {(uint32_t)c->cap, 0u};   // hml_model: cap, halted (adjacent)
    static_assert(offsetof(hml_model, halted) == offsetof(hml_model, cap) + sizeof(uint32_t), "cap and halted are written together");
    if (!c->probes) { c->d_eprobe.free(); c->d_aprobe.free(); }   // (switched off: hml_enable_probes allocates them again, at the capacity of its day)
    if (int r = alloc_capacity_buffers(c, CAPBUF_BLOCKS | (c->model_set ? CAPBUF_SWEEP | (c->probes ? CAPBUF_PROBES : 0) : 0))) { c->cap = old_cap; return r; }
    HIPCHK(hipMemcpyAsync(&c->d_mdl->cap, words, sizeof words, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->h_B[2] = 0u;
    c->blocks_valid = false;
    c->hint_stale = false;      // (h_B[0] holds the count the halted enumeration found)
    c->grown++;
    return 0;
}

// The stream is idle and no sweep was left behind: a chain whose enumeration found more blocks than its buffers hold (it halts
// on the device, hml_state.h) gets larger buffers, and the sweeps it skipped - everything enqueued since the model's sweep
// counter stopped - run again, in order, with their recording flags.  Same results as with room from the start: a halted sweep
// changes nothing but scratch.
int hml_settle(hml_ctx* c) {
    for (int round = 0; round < 64; ++round) {
        HIPCHK(hipStreamSynchronize(c->stream));
        if (!chain_halted(c)) { c->sweep_log.clear(); c->log_base = c->requested; return 0; }
        const uint64_t needed = c->h_B[2];
        if (c->cap >= c->T) return set_err(HML_ERR_HIP, "internal error: a chain with full block capacity halted");
        std::vector<uint8_t> pending;
        unsigned long long base = c->log_base;
        if (c->model_set) {
            hml_model m;
            if (int r = fetch_model(c, &m)) return r;
            // (the log starts at log_base sweeps; what the counter says beyond that ran, the rest did not)
            const uint64_t ran = m.sweeps >= c->log_base ? m.sweeps - c->log_base : 0;
            if (ran < c->sweep_log.size()) pending.assign(c->sweep_log.begin() + ran, c->sweep_log.end());
            base = m.sweeps;
        }
        if (int r = grow_capacity(c, needed)) return r;   // (log and base as they were: the call can be made again)
        // the log now holds exactly the sweeps that have to run (again): the model's counter tells how far they got
        c->sweep_log = pending;
        c->log_base = base;
        bool halted_again = false;
        for (size_t i = 0; i < pending.size() && !halted_again; ++i) {
            const char method = (pending[i] & 1) ? HML_METHOD_MIXTURE : HML_METHOD_FB;
            const bool record = (pending[i] & 2) != 0;
            if (int r = c->kt->sweep(c, method, record)) return r;
            if (record && c->cb) {   // a recorded sweep the caller wants to see: it happens now (or, halted again, in the next round)
                HIPCHK(hipStreamSynchronize(c->stream));
                halted_again = chain_halted(c);
                if (!halted_again) {
                    if (int r = check_device_error(c)) return r;
                    // (hml.h: the callback is told the sweep's index in its hml_iterate call, not its place in this list)
                    const unsigned long long ordinal = c->log_base + i;
                    c->cb(c, ordinal >= c->call_base ? (uint64_t)(ordinal - c->call_base) : 0u, c->cb_user);
                }
            }
        }
    }
    return set_err(HML_ERR_HIP, "internal error: the block capacity did not settle");
}

extern "C" {

// ---------------------------------------------------------------------------------------- model
int hml_set_model(hml_ctx* c, int K, const float nig4[4], float a_off, float a_diag, float pi_alpha, int self_trans) {
    if (!c || !c->loaded) return set_err(HML_ERR_ARG, "no observations loaded");
    if (K < 2) return set_err(HML_ERR_MODEL, "Requested parameters would yield an HMM with less than 2 states!");
    if (K > HML_CAP_K) return set_err(HML_ERR_ARG, "number of states must be in [2,64]");
    if (c->model_set) return set_err(HML_ERR_ARG, "model already set");
    if (c->D > 1 && c->P == 0) {   // the number of parameters follows from K = P^D
        for (int pp = 2; pp <= K; ++pp) { long k = 1; for (int d = 0; d < c->D; ++d) k *= pp; if (k == K) { c->P = pp; break; } if (k > K) break; }
        if (c->P == 0) return set_err(HML_ERR_ARG, "number of states must be (number of parameters)^(data dimensions)");
    }
    if (c->P > 0) {
        long k = 1;
        for (int d = 0; d < c->D; ++d) k *= c->P;
        if (k != K) return set_err(HML_ERR_ARG, "number of states must be (number of parameters)^(data dimensions)");
    }
    if (!(nig4[0] > 0)) return set_err(HML_ERR_MODEL, "Alpha (" + std::to_string(nig4[0]) + ") must be positive!");
    if (!(nig4[1] > 0)) return set_err(HML_ERR_MODEL, "Beta (" + std::to_string(nig4[1]) + ") must be positive!");
    if (!(nig4[3] > 0)) return set_err(HML_ERR_MODEL, "Nu (" + std::to_string(nig4[3]) + ")must be positive!");
    // more than 16 states: the kernels that take the number of states at run time (hml_k_wide.h; HML_WIDE=1: from 2 states - tests)
    c->wide = !c->compat && (K > HML_MAX_K || (getenv("HML_WIDE") && atoi(getenv("HML_WIDE")) != 0));
    // the context's path, chosen ONCE, before anything is allocated (a development build knows one K only; the other two take K at run time)
    c->kt = (c->compat || c->wide) ? rtk_tab(c->wide) : ktab(K);
    if (!c->kt) return set_err(HML_ERR_ARG, "number of states must be in [2,16]");
    if (int r = ctx_bind(c)) return r;
    c->K = K;
    // the parameter kernel's tree over 16 workgroups (hml_k_params.h) from 8 states: it reads 2 K x 8 KB of group partials -
    // config 4's sweep (10 states) 0.0938 -> 0.0869 ms, config 3's (5 states) unchanged either way
    if (!getenv("HML_PARAMS_SPREAD")) c->knobs.params_spread = K >= 8;
    const uint64_t T = c->T;
    if (int r = alloc_capacity_buffers(c, CAPBUF_SWEEP)) return r;

    hml_model m;
    memset(&m, 0, sizeof m);
    m.K = K; m.self_trans = self_trans ? 1 : 0; m.dynamic = 1; m.T = (uint32_t)T;
    m.D = c->D; m.P = c->P > 0 ? c->P : K; m.stat_stride = T;
    m.cap = (uint32_t)c->cap;
    for (int st = 0; st < K; ++st) {   // reversed P-ary digits (Mapping.hpp:92-103)
        int nn = st;
        for (int d = 0; d < HML_MAX_D; ++d) { m.map[st][d] = (uint8_t)(d < c->D ? nn % m.P : 0); nn /= m.P; }
    }
    for (int i = 0; i < 4; ++i) m.nig_prior[i] = nig4[i];
    m.a_off = a_off; m.a_diag = a_diag; m.pi_alpha = pi_alpha;
    m.key = hml_make_key(c->seed, c->chain);
    for (int k = 0; k < K; ++k) {
        for (int i = 0; i < 4; ++i) m.nig_post[k][i] = nig4[i];
        m.dirPi[k] = pi_alpha;
        m.pi[k] = 1.0f / K;
        for (int j = 0; j < K; ++j) { m.dirA[k * K + j] = (k == j) ? a_diag : a_off; m.A[k * K + j] = 1.0f / K; }
    }
    m.max_state_recorded = -1;
    m.tre_fused = (c->knobs.tre_fused && c->D == 1) ? 1u : 0u;
    m.tre_hi_shift = 17u; m.tre_lo_shift = 20u;
    if (const char* e = getenv("HML_TRE_REFIT_SHIFTS")) { unsigned a = 17, b = 20; if (sscanf(e, "%u,%u", &a, &b) == 2 && a < 32 && b < 32) { m.tre_hi_shift = a; m.tre_lo_shift = b; } }
    m.fwd_W0 = (uint32_t)c->fwdW;
    m.fwd_W = m.fwd_W_burnin = (uint32_t)std::max(c->fwdW, c->fwdW_init);
    if (c->compat || c->wide) { m.fwd_W = 64u; m.fwd_W0 = c->wide ? (uint32_t)c->rtk.wide_w0 : 32u; }
    m.wl_bwd_W = 64u; m.wl_bwd_quiet = 0u; m.wl_retry = 0u; m.wl_W_need = 0u; m.wl_need_age = 0u;   // the chunked lane-per-state kernels' own policy (hml_chunk_warmup_adapt)
    m.fwd_burnin_sweeps = c->fwd_burnin_sweeps;
    m.fwd_quiet_need = c->fwd_quiet_need;
    m.n_spans = c->n_spans;
    // the parameter kernel stamps its stages only when they will be printed (hml_sync): the flag travels with the model
    m.dbg_t[HML_PARAMS_DBG_FLAG] = getenv("HML_PARAMS_DEBUG") ? 1ull : 0ull;
    // keep the block count of an earlier enumeration (autoprior) out of the model: B = 0
    HIPCHK(hipMemcpyAsync(c->d_mdl, &m, sizeof m, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->dynamic = true;
    c->hint_stale = true;
    if (c->compat) {
        // reference-compatible mode (hml_k_compat.h): the reference's engine, seeded like `rng_t RNG(seed)` (main.cpp:107-108).
        // Chain 0 is the reference's run at this seed; further chains of a run (`-chains N`, chain ids 1, 2, ...) are the
        // reference's runs at seed + chain id - N copies of one chain would pool to N times its marginals.
        hml_mt_state h;
        hml_mt_seed(&h, c->seed + (uint64_t)c->chain);
        HIPCHK(c->d_mt.alloc(sizeof(hml_mt_state)));
        HIPCHK(hipMemcpyAsync(c->d_mt.get(), &h, sizeof h, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    c->kt->params(c, 2);   // Theta's constructor samples once from the prior (src/Theta.hpp:126-127)
    KLAUNCH_CHECK();
    c->model_set = true;
    return 0;
}

int hml_sample_prior(hml_ctx* c) {
    if (!c || !c->model_set) return set_err(HML_ERR_ARG, "model not set");
    if (int r = ctx_bind(c)) return r;
    if (int r = settle_if_limited(c)) return r;
    c->kt->params(c, 1);
    KLAUNCH_CHECK();
    if (c->dynamic) c->blocks_valid = false;
    c->hint_stale = true;
    return 0;
}

HML_KERNEL __launch_bounds__(64) void hml_k_set_self_trans(hml_model* mdl, int on) {
    if (threadIdx.x == 0) mdl->self_trans = on;
}

int hml_set_self_transitions(hml_ctx* c, int on) {
    if (!c || !c->model_set) return set_err(HML_ERR_ARG, "model not set");
    if (int r = ctx_bind(c)) return r;
    if (int r = settle_if_limited(c)) return r;
    hipLaunchKernelGGL(hml_k_set_self_trans, dim3(1), dim3(64), 0, c->stream, c->d_mdl, on ? 1 : 0);
    KLAUNCH_CHECK();
    drop_graph(c);
    return 0;
}

int hml_set_static_blocks(hml_ctx* c) {
    if (!c || !c->model_set) return set_err(HML_ERR_ARG, "model not set");
    if (int r = ctx_bind(c)) return r;
    if (int r = settle_if_limited(c)) return r;
    hipLaunchKernelGGL(hml_k_set_dynamic, dim3(1), dim3(64), 0, c->stream, c->d_mdl, 0, 1);
    KLAUNCH_CHECK();
    c->dynamic = false;
    drop_graph(c);   // (a captured sweep holds the block launches or not)
    if (!cap_limited(c)) {
        if (int r = launch_compact(c, false, 0.0f)) return r;
    } else {
        // a context with a reduced block capacity (attached chains, option max_blocks): the enumeration at the model's
        // threshold may find more blocks than the buffers hold - it then writes nothing and halts the chain.  The structure
        // is only valid once an enumeration has fitted, so wait for it and grow like enumerate_blocks_sync (ADVICE round 4:
        // static sweeps enqueued behind a halted enumeration ran as no-ops until the host noticed)
        bool fitted = false;
        for (int round = 0; round < 64 && !fitted; ++round) {
            if (int r = launch_compact(c, false, 0.0f)) return r;
            HIPCHK(hipStreamSynchronize(c->stream));
            fitted = !chain_halted(c);
            if (!fitted) { if (int r = grow_capacity(c, c->h_B[2])) return r; }
        }
        if (!fitted) return set_err(HML_ERR_HIP, "internal error: the block capacity did not settle");
        refresh_hint(c);
    }
    c->blocks_valid = true;
    return 0;
}

int hml_set_dynamic(hml_ctx* c, int on) {
    if (!c || !c->model_set) return set_err(HML_ERR_ARG, "model not set");
    if (int r = ctx_bind(c)) return r;
    if (int r = settle_if_limited(c)) return r;
    hipLaunchKernelGGL(hml_k_set_dynamic, dim3(1), dim3(64), 0, c->stream, c->d_mdl, on ? 1 : 0, on ? 1 : 0);
    KLAUNCH_CHECK();
    c->dynamic = on != 0;
    drop_graph(c);
    if (on) { c->blocks_valid = false; c->hint_stale = true; }
    return 0;
}

int hml_set_recording(hml_ctx* c, int marginals, hml_record_cb cb, void* user) {
    if (!c) return set_err(HML_ERR_ARG, "null context");
    c->rec_marginals = marginals != 0;
    c->cb = cb; c->cb_user = user;
    return 0;
}

static int set_recorder(hml_ctx* c, int kind, int on) {
    if (!c) return set_err(HML_ERR_ARG, "null context");
    c->rec[kind].on = on != 0;
    if (on) c->rec[kind].asked = true;
    // (recorded sweeps are never replayed from a captured graph - hml_iterate - but a graph captured under the other setting goes anyway)
    if (c->graph_exec) { if (int r = ctx_bind(c)) return r; drop_graph(c); }
    return 0;
}
int hml_set_level_recording(hml_ctx* c, int on) { return set_recorder(c, HML_REC_LEVELS, on); }
int hml_set_break_recording(hml_ctx* c, int on) { return set_recorder(c, HML_REC_BREAKS, on); }

int hml_set_level_bands(hml_ctx* c, int n_edges, const float* edges) {
    if (!c) return set_err(HML_ERR_ARG, "null context");
    // (as in hml_set_level_recording: a graph captured under the other setting goes)
    if (c->graph_exec) { if (int r = ctx_bind(c)) return r; drop_graph(c); }
    if (n_edges == 0) { c->rec[HML_REC_BANDS].on = false; return 0; }   // (what was accumulated stays, and so do its edges)
    if (!edges) return set_err(HML_ERR_ARG, "null argument");
    if (const char* why = band_edges_fault(n_edges, edges)) return set_err(HML_ERR_ARG, why);
    if (c->model_set && (uint64_t)c->D * (uint64_t)(n_edges + 1) > HML_CAP_K)
        return set_err(HML_ERR_ARG, "level bands: the data dimensions times (edges + 1) exceed 64 columns");
    if (!same_band_edges(c, n_edges, edges) && c->rec[HML_REC_BANDS].d_acc) {
        // buffers of other edges: they go if they hold nothing
        if (int r = ctx_bind(c)) return r;
        if (int r = hml_settle(c)) return r;
        hml_model m; if (int r = fetch_model(c, &m)) return r;
        if (m.n_bands_recorded != 0ull) return set_err(HML_ERR_ARG, "level bands were already recorded under other edges: they cannot be changed any more");
        hml_recorder& rec = c->rec[HML_REC_BANDS];
        rec.d_acc.free();
        rec.d_boundary.free();
    }
    c->n_band_edges = n_edges;
    memcpy(c->band_edges, edges, (size_t)n_edges * sizeof(float));
    c->rec[HML_REC_BANDS].on = c->rec[HML_REC_BANDS].asked = true;
    return 0;
}

int hml_get_level_bands(hml_ctx* c, int* n_edges, float* edges) {
    if (!c || !n_edges) return set_err(HML_ERR_ARG, "null argument");
    *n_edges = c->n_band_edges;
    if (edges) memcpy(edges, c->band_edges, (size_t)c->n_band_edges * sizeof(float));
    return 0;
}

// The regions of the joint posteriors (hml_k_regions.h).  What can be told without the trace is refused here, the rest -
// a region beyond the trace that is loaded later - by the first recorded sweep (regions_fault).
int hml_set_regions(hml_ctx* c, uint64_t n, const uint32_t* start, const uint32_t* end, int n_edges, const float* edges) {
    if (!c) return set_err(HML_ERR_ARG, "null context");
    // (as in hml_set_level_recording: a graph captured under the other setting goes)
    if (c->graph_exec) { if (int r = ctx_bind(c)) return r; drop_graph(c); }
    if (n == 0) { c->rg.on = false; return 0; }   // (what was accumulated stays, and so do the regions and their edges)
    if (!start || !end || (n_edges > 0 && !edges)) return set_err(HML_ERR_ARG, "null argument");
    if (n > (1ull << 22)) return set_err(HML_ERR_ARG, "regions: 1 to 2^22 regions");
    if (n_edges < 0) return set_err(HML_ERR_ARG, "level bands take 1 to 31 edges");
    if (n_edges > 0) { if (const char* why = band_edges_fault(n_edges, edges)) return set_err(HML_ERR_ARG, why); }
    if (c->model_set && (uint64_t)c->D * (uint64_t)(n_edges + 1) > HML_CAP_K)
        return set_err(HML_ERR_ARG, "regions: the data dimensions times (edges + 1) exceed 64 columns");
    for (uint64_t r = 0; r < n; ++r)
        if (!(start[r] < end[r]) || (c->loaded && (uint64_t)end[r] > c->T)) {
            char buf[200];
            if (c->loaded) snprintf(buf, sizeof buf, "regions: region %llu, [%u, %u), does not lie inside the %llu positions of the trace", (unsigned long long)r, start[r], end[r], (unsigned long long)c->T);
            else snprintf(buf, sizeof buf, "regions: region %llu, [%u, %u), is empty", (unsigned long long)r, start[r], end[r]);
            return set_err(HML_ERR_ARG, buf);
        }
    if (!same_regions(c, n, start, end, n_edges, edges)) {
        if (c->rg.d_acc) {
            // buffers of other regions or edges: they go if they hold nothing
            if (int r = ctx_bind(c)) return r;
            if (int r = hml_settle(c)) return r;
            unsigned long long N = 0;
            HIPCHK(hipMemcpy(&N, &c->d_mdl->n_regions_recorded, sizeof N, hipMemcpyDeviceToHost));
            if (N != 0ull) return set_err(HML_ERR_ARG, "regions were already recorded under other regions or edges: they cannot be changed any more");
            c->rg.d_start.free(); c->rg.d_end.free(); c->rg.d_chunks.free(); c->rg.d_acc.free();
        }
        c->rg.start.assign(start, start + n);
        c->rg.end.assign(end, end + n);
        c->rg.n_edges = n_edges;
        memset(c->rg.edges, 0, sizeof c->rg.edges);
        if (n_edges > 0) memcpy(c->rg.edges, edges, (size_t)n_edges * sizeof(float));
        c->rg.checked = c->loaded && c->model_set;
    }
    c->rg.on = c->rg.asked = true;
    return 0;
}

int hml_get_regions(hml_ctx* c, uint64_t* n, uint32_t* start, uint32_t* end, int* n_edges, float* edges) {
    if (!c || !n) return set_err(HML_ERR_ARG, "null argument");
    *n = c->rg.start.size();
    if (start) memcpy(start, c->rg.start.data(), c->rg.start.size() * sizeof(uint32_t));
    if (end) memcpy(end, c->rg.end.data(), c->rg.end.size() * sizeof(uint32_t));
    if (n_edges) *n_edges = c->rg.n_edges;
    if (edges) memcpy(edges, c->rg.edges, (size_t)c->rg.n_edges * sizeof(float));
    return 0;
}

int hml_enable_probes(hml_ctx* c, int on) {
    if (!c || !c->model_set) return set_err(HML_ERR_ARG, "model not set");
    if (int r = ctx_bind(c)) return r;
    if (int r = settle_if_limited(c)) return r;
    if (on && !c->d_aprobe) { if (int r = alloc_capacity_buffers(c, CAPBUF_PROBES)) return r; }   // (the second of the pair: both are there)
    c->probes = on != 0;
    return 0;
}

// ---------------------------------------------------------------------------------------- sweeps
}  // extern "C"

int hml_ctx_ensure_marginal_buffers(hml_ctx* c) { return ensure_marginal_buffers(c); }

#include "hml_rtk_sweep.hpp"   // sweep_compat, sweep_wide and their tables

// One sweep of a chain and, on a recorded sweep with a callback: wait, settle if the chain halted (that runs the sweep again
// and calls back), check the device error, call back.
static int sweep_step(hml_ctx* c, char method, bool record, uint64_t i) {
    log_sweep(c, method, record);
    if (int r = c->kt->sweep(c, method, record)) return r;
    if (!(record && c->cb)) return 0;
    HIPCHK(hipStreamSynchronize(c->stream));
    if (chain_halted(c)) return hml_settle(c);
    if (int r = check_device_error(c)) return r;
    c->cb(c, i, c->cb_user);
    return 0;
}

// HML_USE_GRAPH: replay a captured sweep.  It is captured again when there is none, when the plan of the coming sweep differs
// from the one it was captured under (hml_sweep_plan.h: method, geometry, block path, scan variant, ...), when the grid hint left
// [captured / 2, captured], or when the fused trellis path would take another chunk length.  *replayed: the sweep is enqueued.
static int replay_captured(hml_ctx* c, char method, bool* replayed) {
    *replayed = false;
    const uint32_t hint = c->B_hint;
    const hml_sweep_plan plan = plan_of(c, method == HML_METHOD_MIXTURE, c->h_B[1] != 0u);
    if (plan.trellis && tre_wants_measurement(c, hint)) return 0;   // (a measuring sweep runs outside any graph)
    bool unused = false;
    const bool stale = !c->graph_exec || !(plan == c->captured.plan) || hint > c->captured.hint || hint * 2u < c->captured.hint ||
                       (plan.trellis && c->captured.tre_L != tre_pick_L(c, hint, true, &unused));
    if (stale && hint) {
        drop_graph(c);
        hipGraph_t g = nullptr;
        HIPCHK(hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
        // whatever happens below, the stream must leave capture mode (a failure in between would otherwise
        // make every later call on this context fail) and a partial graph must not stay behind
        int rr = c->kt->sweep(c, method, false);
        const hipError_t ec = hipStreamEndCapture(c->stream, &g);
        if (rr || ec != hipSuccess) {
            if (g) hipGraphDestroy(g);
            (void)hipGetLastError();
            return rr ? rr : set_err(HML_ERR_HIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(ec));
        }
        const hipError_t ei = hipGraphInstantiate(&c->graph_exec, g, nullptr, nullptr, 0);
        hipGraphDestroy(g);
        if (ei != hipSuccess) { c->graph_exec = nullptr; return set_err(HML_ERR_HIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(ei)); }
        c->captured.plan = plan; c->captured.hint = c->B_hint; c->captured.tre_L = c->tre_last_L;
    }
    if (!c->graph_exec) return 0;
    log_sweep(c, method, false);
    HIPCHK(hipGraphLaunch(c->graph_exec, c->stream));
    if (plan.trellis) c->tre_dense_sweeps++;
    *replayed = true;
    return 0;
}

extern "C" {

int hml_iterate(hml_ctx* c, char method, uint64_t iterations, uint64_t thinning) {
    if (!c || !c->model_set) return set_err(HML_ERR_ARG, "model not set");
    if (method != HML_METHOD_FB && method != HML_METHOD_MIXTURE)
        return set_err(HML_ERR_ARG, std::string("Unknown sampling type ") + method + "!");
    if (int r = ctx_bind(c)) return r;
    c->call_base = c->requested;
    if (int r = pooled_refusal(c, thinning > 0 && thinning <= iterations, "this context")) return r;   // (before anything is enqueued: a sweep is not abandoned half-way)
    if (int r = hml_history_ensure(c, iterations)) return r;   // (room for the rows of this call, before anything is enqueued)
    for (uint64_t i = 0; i < iterations; ++i) {
        const bool record = thinning > 0 && ((i + 1) % thinning == 0);
        // a chain with a reduced block capacity that halted (hml_state.h): larger buffers, the skipped sweeps again - then on
        if (chain_halted(c)) { if (int r = hml_settle(c)) return r; }
        refresh_hint(c);
        if (c->use_graph && !c->compat && !record && !c->profiling && !c->probes && (c->dynamic || c->blocks_valid)) {
            bool replayed = false;
            if (int r = replay_captured(c, method, &replayed)) return r;
            if (replayed) continue;
        }
        if (int r = sweep_step(c, method, record, i)) return r;
    }
    return 0;
}

}  // extern "C"

extern "C" int hml_iterate_many(hml_ctx* const* cs, int n, char method, uint64_t iterations, uint64_t thinning) {
    if (!cs || n < 1) return set_err(HML_ERR_ARG, "no contexts");
    for (int i = 0; i < n; ++i) if (!cs[i] || !cs[i]->model_set) return set_err(HML_ERR_ARG, "model not set");
    if (method != HML_METHOD_FB && method != HML_METHOD_MIXTURE) return set_err(HML_ERR_ARG, std::string("Unknown sampling type ") + method + "!");
    for (int i = 0; i < n; ++i) cs[i]->call_base = cs[i]->requested;
    // room for the rows of this call in every chain that keeps a history - the batches and the chain-by-chain tail - before anything is enqueued
    for (int i = 0; i < n; ++i) if (cs[i]->hist.on) { if (int r = ctx_bind(cs[i])) return r; if (int r = hml_history_ensure(cs[i], iterations)) return r; }
    uint64_t done = 0;
    while (done < iterations && many_eligible(cs, n, method)) {
        if (int r = ctx_bind(cs[0])) return r;
        // everything the chains have enqueued on their own streams comes first (a chain with a reduced block capacity catches up
        // on what it skipped: hml_settle); a block count that predates the current parameters is refreshed chain by chain
        // (sweep_k's first-sweep rule)
        for (int i = 0; i < n; ++i) {
            hml_ctx* c = cs[i];
            if (int r = settle_if_limited(c)) return r;
            if (c->hint_stale) { launch_compact_pair(c, 0, 0.0f); KLAUNCH_CHECK(); }
            HIPCHK(hipStreamSynchronize(c->stream));
            c->hint_stale = false;
            drop_graph(c);
        }
        uint64_t reached = done;
        if (int r = cs[0]->kt->iterate_many(cs, n, done, iterations, thinning, &reached)) return r;   // (many_eligible: a table that has one)
        // the other chains' streams continue behind the batch
        hipEvent_t ev = ev_get(cs[0]);
        HIPCHK(hipEventRecord(ev, cs[0]->stream));
        for (int i = 1; i < n; ++i) HIPCHK(hipStreamWaitEvent(cs[i]->stream, ev, 0));
        cs[0]->ev_pool.push_back(ev);
        if (reached == iterations) return 0;
        HIPCHK(hipStreamSynchronize(cs[0]->stream));
        // the batch stopped early: a chain halted (its blocks outgrew its buffers - the loop's first step lets it catch up, then
        // the batch goes on) or left the strongly compressed regime (chain by chain from here)
        bool halted = false;
        for (int i = 0; i < n; ++i) halted = halted || chain_halted(cs[i]);
        const bool progress = reached > done;
        done = reached;
        if (!halted && !progress) break;
        if (!halted) { bool sparse = true; for (int i = 0; i < n; ++i) sparse = sparse && many_sparse(cs[i]); if (!sparse) break; }
    }
    for (int i = 0; i < n; ++i) if (int r = settle_if_limited(cs[i])) return r;
    // not batched (different shapes or devices, mixture sweeps, weakly compressed or reference-compatible chains): sweep by
    // sweep in turn, so that recorded sweeps stay aligned across the chains
    for (uint64_t i = done; i < iterations; ++i) {
        const bool record = thinning > 0 && ((i + 1) % thinning == 0);
        for (int k = 0; k < n; ++k) {
            hml_ctx* c = cs[k];
            if (int r = ctx_bind(c)) return r;
            if (int r = pooled_refusal(c, record, "a context")) return r;
            if (chain_halted(c)) { if (int r = hml_settle(c)) return r; }
            if (int r = sweep_step(c, method, record, i)) return r;
        }
    }
    return 0;
}

extern "C" {

int hml_set_option(hml_ctx* c, const char* name, int value) {
    if (!c || !name) return set_err(HML_ERR_ARG, "null argument");
    if (std::string(name) == "weight_keys") {
        if (c->loaded) return set_err(HML_ERR_ARG, "weight_keys must be set before the observations are loaded");
        c->knobs.use_keys = value != 0;
        c->knobs.summary_always = value == 2;
        return 0;
    }
    if (std::string(name) == "max_blocks") {   // block capacity of the per-block buffers (hml_ctx.hpp)
        if (c->loaded) return set_err(HML_ERR_ARG, "max_blocks must be set before the observations are loaded");
        if (value < 0) return set_err(HML_ERR_ARG, "max_blocks: a number of blocks, or 0 for the default");
        c->cap_opt = (uint64_t)value;
        return 0;
    }
    if (std::string(name) == "fused_blocks") {
        c->knobs.fused_blocks = value != 0;
        c->knobs.fused_keep = value == 2;
        drop_graph(c);
        return 0;
    }
    if (std::string(name) == "compat") {   // the reference-compatible mode (hml_k_compat.h): before hml_set_model
        if (c->model_set) return set_err(HML_ERR_ARG, "compat must be set before the model");
        c->compat = value != 0;
        return 0;
    }
    if (std::string(name) == "trellis_L") {   // chunk length of the fused trellis path: 0 = measured, else a multiple of 32 up to HML_TRE_MAX_L
        if (value < 0 || value > HML_TRE_MAX_L || value % 32) return set_err(HML_ERR_ARG, "trellis_L: 0 or a multiple of 32 up to 1024");
        c->tre_L = (uint32_t)value;
        return 0;
    }
    // the launch geometry of the chunked passes of exact inference (hml_infer.hip): never part of a result
    const struct { const char* pass; hml_ctx::chunked_pass* p; } passes[] = {{"viterbi", &c->vit}, {"posterior", &c->post}, {"sample", &c->samp}};
    for (const auto& e : passes) {
        const std::string pass(e.pass), opt(name);
        if (opt == pass + "_W" || opt == pass + "_L") {
            if (value < 0 || value > (1 << 20)) return set_err(HML_ERR_ARG, opt + ": a number of blocks up to 2^20, or 0 for the default");
            (opt.back() == 'W' ? e.p->W : e.p->L) = (uint32_t)value;
            return 0;
        }
        if (opt == pass + "_rounds") {
            if (value < 0 || value > 16) return set_err(HML_ERR_ARG, opt + ": 0 to 16 parallel repair rounds");
            e.p->rounds = (uint32_t)value;
            return 0;
        }
    }
    return set_err(HML_ERR_ARG, std::string("unknown option ") + name);
}

int hml_sync(hml_ctx* c) {
    if (!c) return set_err(HML_ERR_ARG, "null context");
    if (int r = ctx_bind(c)) return r;
    if (int r = hml_settle(c)) return r;   // (synchronises; a halted chain grows and catches up)
    if (c->d_dbg && getenv("HML_FUSED_DEBUG") && atoi(getenv("HML_FUSED_DEBUG")) == 2) {
        // the many-chain block kernel's stamps (8 words per workgroup): start | phase A done | first gathers requested | offsets known | end
        std::vector<unsigned long long> h(4096 * 8);
        hipMemcpy(h.data(), c->d_dbg, h.size() * 8, hipMemcpyDeviceToHost);
        uint32_t n = 0; while (n < 4096 && h[n * 8]) ++n;
        unsigned long long t0 = ~0ull; for (uint32_t i = 0; i < n; ++i) t0 = std::min(t0, h[i * 8]);
        double mx[5] = {0, 0, 0, 0, 0}, av[5] = {0, 0, 0, 0, 0};
        if (n) for (uint32_t i = 0; i < n; ++i) for (int k = 0; k < 5; ++k) { const double d = (double)(h[i * 8 + k] - t0) * 0.01; mx[k] = std::max(mx[k], d); av[k] += d / n; }
        if (n) fprintf(stderr, "[fused-many dbg] n=%u start avg %.2f max %.2f | phaseA avg %.2f max %.2f | requested avg %.2f max %.2f | offsets avg %.2f max %.2f | end avg %.2f max %.2f (us)\n",
                n, av[0], mx[0], av[1], mx[1], av[2], mx[2], av[3], mx[3], av[4], mx[4]);
        if (n) for (uint32_t i : {0u, n / 4, n / 2, n - 1}) if (i < n) fprintf(stderr, "   wg %u: %.2f %.2f %.2f %.2f %.2f | wavefront 0: parameters in LDS %.2f, weights arrived %.2f, its lists done %.2f\n", i, (h[i*8]-t0)*0.01, (h[i*8+1]-t0)*0.01, (h[i*8+2]-t0)*0.01, (h[i*8+3]-t0)*0.01, (h[i*8+4]-t0)*0.01,
                                                                                  (h[i*8+5]-t0)*0.01, (h[i*8+6]-t0)*0.01, (h[i*8+7]-t0)*0.01);
    } else if (c->d_dbg) {
        std::vector<unsigned long long> h(4096 * 4);
        hipMemcpy(h.data(), c->d_dbg, h.size() * 8, hipMemcpyDeviceToHost);
        const uint32_t n = (uint32_t)std::min<uint64_t>(4096, (c->T + HML_FUSED_SUB_POSITIONS - 1) / HML_FUSED_SUB_POSITIONS);
        unsigned long long t0 = ~0ull; for (uint32_t i = 0; i < n; ++i) if (h[i * 4]) t0 = std::min(t0, h[i * 4]);
        double mx[4] = {0, 0, 0, 0}, av[4] = {0, 0, 0, 0};
        for (uint32_t i = 0; i < n; ++i) for (int k = 0; k < 4; ++k) { const double d = (double)(h[i * 4 + k] - t0) * 0.01; mx[k] = std::max(mx[k], d); av[k] += d / n; }
        fprintf(stderr, "[fused dbg] n=%u start avg %.2f max %.2f | phaseA avg %.2f max %.2f | offsets avg %.2f max %.2f | end avg %.2f max %.2f (us)\n", n, av[0], mx[0], av[1], mx[1], av[2], mx[2], av[3], mx[3]);
        { uint32_t late = 0, first_late = n; for (uint32_t i = 0; i < n; ++i) if ((h[i * 4] - t0) * 0.01 > 2.0) { ++late; first_late = std::min(first_late, i); }
          fprintf(stderr, "   late starters: %u, first index %u\n", late, first_late); }
        for (uint32_t i : {0u, n / 4, n / 2, n - 1}) fprintf(stderr, "   wg %u: %.2f %.2f %.2f %.2f\n", i, (h[i*4]-t0)*0.01, (h[i*4+1]-t0)*0.01, (h[i*4+2]-t0)*0.01, (h[i*4+3]-t0)*0.01);
    }
    if (c->model_set && getenv("HML_PARAMS_DEBUG")) {
        hml_model m;
        // (the kernel stamps only when the model carries the flag, which hml_set_model takes from the same variable)
        if (fetch_model(c, &m) == 0 && m.dbg_t[HML_PARAMS_DBG_FLAG] == 0ull) {
            fprintf(stderr, "[params dbg] no stamps: HML_PARAMS_DEBUG was not set when the model was set up\n");
        } else if (fetch_model(c, &m) == 0) {
            fprintf(stderr, "[params dbg] us since the kernel's start: accumulators read %.2f | tree %.2f | theta drawn %.2f | A gammas %.2f | barrier %.2f | end %.2f\n",
                    (m.dbg_t[1] - m.dbg_t[0]) * 0.01, (m.dbg_t[2] - m.dbg_t[0]) * 0.01, (m.dbg_t[3] - m.dbg_t[0]) * 0.01, (m.dbg_t[4] - m.dbg_t[0]) * 0.01,
                    (m.dbg_t[5] - m.dbg_t[0]) * 0.01, (m.dbg_t[6] - m.dbg_t[0]) * 0.01);
            fprintf(stderr, "[params dbg]   theta's gamma core + normal drawn %.2f | last wavefront's tree %.2f\n", (m.dbg_t[7] - m.dbg_t[0]) * 0.01, (m.dbg_t[8] - m.dbg_t[0]) * 0.01);
        }
    }
    if (c->model_set) return check_device_error(c);
    return 0;
}

// ---------------------------------------------------------------------------------------- probes

static int current_B(hml_ctx* c, uint32_t* B) {
    HIPCHK(hipMemcpyAsync(c->h_B, &c->d_mdl->B, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    *B = *c->h_B;
    return 0;
}

int hml_get_num_blocks(hml_ctx* c, uint64_t* B) {
    NEED_LOADED();
    uint32_t b; if (int r = current_B(c, &b)) return r;
    *B = b; return 0;
}
int hml_get_blocks(hml_ctx* c, uint32_t* starts) {
    NEED_LOADED();
    uint32_t b; if (int r = current_B(c, &b)) return r;
    HIPCHK(hipMemcpy(starts, c->d_starts, ((uint64_t)b + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return 0;
}
int hml_get_block_stats(hml_ctx* c, float* sum, float* sum_sq) {
    NEED_LOADED();
    uint32_t b; if (int r = current_B(c, &b)) return r;
    std::vector<float2> v(b);
    for (int d = 0; d < c->D; ++d) {   // one plane per data dimension
        HIPCHK(hipMemcpy(v.data(), c->d_bstat + (uint64_t)d * c->T, (uint64_t)b * sizeof(float2), hipMemcpyDeviceToHost));
        for (uint32_t i = 0; i < b; ++i) { sum[(uint64_t)d * b + i] = v[i].x; sum_sq[(uint64_t)d * b + i] = v[i].y; }
    }
    return 0;
}
int hml_get_states(hml_ctx* c, int16_t* q) {
    NEED_MODEL();
    uint32_t b; if (int r = current_B(c, &b)) return r;
    HIPCHK(hipMemcpy(q, c->d_q, (uint64_t)b * sizeof(int16_t), hipMemcpyDeviceToHost));
    return 0;
}
int hml_get_theta(hml_ctx* c, float* mean_var) {
    NEED_MODEL();
    hml_model m; if (int r = fetch_model(c, &m)) return r;
    for (int k = 0; k < m.P; ++k) { mean_var[2 * k] = m.mu[k]; mean_var[2 * k + 1] = m.var[k]; }   // one pair per parameter
    return 0;
}
int hml_get_dimensions(hml_ctx* c, int* D, int* P) {
    if (!c) return set_err(HML_ERR_ARG, "null context");
    if (D) *D = c->D;
    if (P) *P = c->P > 0 ? c->P : c->K;
    return 0;
}
int hml_get_transitions(hml_ctx* c, float* A, float* pi) {
    NEED_MODEL();
    hml_model m; if (int r = fetch_model(c, &m)) return r;
    if (A) memcpy(A, m.A, (size_t)c->K * c->K * sizeof(float));
    if (pi) memcpy(pi, m.pi, (size_t)c->K * sizeof(float));
    return 0;
}
int hml_set_parameters(hml_ctx* c, const float* mean_var, const float* A, const float* pi) {
    NEED_MODEL();
    hml_model m; if (int r = fetch_model(c, &m)) return r;
    const int K = c->K;
    for (int k = 0; k < m.P; ++k) {
        const float mean = mean_var[2 * k], var = mean_var[2 * k + 1];
        if (!std::isfinite(mean)) return set_err(HML_ERR_MODEL, "Mean (" + std::to_string(mean) + ") must be set to a finite value!");
        if (!std::isfinite(var)) return set_err(HML_ERR_MODEL, "Variance(" + std::to_string(var) + ") must be set to a finite value!");
        if (var <= 0) return set_err(HML_ERR_MODEL, "Variance (" + std::to_string(var) + ") must be positive!");
        m.mu[k] = mean; m.var[k] = var; m.sd[k] = sqrtf(var);
    }
    memcpy(m.A, A, (size_t)K * K * sizeof(float));
    memcpy(m.pi, pi, (size_t)K * sizeof(float));
    HIPCHK(hipMemcpyAsync(c->d_mdl, &m, sizeof m, hipMemcpyHostToDevice, c->stream));
    c->kt->derive(c);
    KLAUNCH_CHECK();
    HIPCHK(hipStreamSynchronize(c->stream));
    if (c->dynamic) c->blocks_valid = false;
    return 0;
}
int hml_get_threshold(hml_ctx* c, float* thr) {
    NEED_MODEL();
    hml_model m; if (int r = fetch_model(c, &m)) return r;
    *thr = m.thr; return 0;
}
int hml_get_block_loglik(hml_ctx* c, float* E) {
    NEED_MODEL();
    if (!c->probes) return set_err(HML_ERR_ARG, "probes are not enabled");
    uint32_t b; if (int r = current_B(c, &b)) return r;
    HIPCHK(hipMemcpy(E, c->d_eprobe, (uint64_t)b * c->K * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}
int hml_get_forward_rows(hml_ctx* c, float* rows) {
    NEED_MODEL();
    if (!c->probes) return set_err(HML_ERR_ARG, "probes are not enabled");
    uint32_t b; if (int r = current_B(c, &b)) return r;
    HIPCHK(hipMemcpy(rows, c->d_aprobe, ((uint64_t)b + 1) * c->K * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}
int hml_get_counts(hml_ctx* c, uint64_t* trans, uint64_t* occ, float* sum, float* sum_sq, uint64_t* nterms) {
    NEED_MODEL();
    hml_model m; if (int r = fetch_model(c, &m)) return r;
    const int K = c->K;
    for (int i = 0; i < K * K; ++i) trans[i] = m.last_trans[i];
    for (int k = 0; k < K; ++k) { occ[k] = m.last_occ[k]; nterms[k] = m.last_occ[k]; sum[k] = m.last_sum[k]; sum_sq[k] = m.last_sumsq[k]; }
    return 0;
}
int hml_get_weights(hml_ctx* c, float* w) {
    NEED_LOADED();
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpy(w, c->d_w, c->T * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}
int hml_get_coefficients(hml_ctx* c, float* cf) {
    NEED_LOADED();
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpy(cf, c->d_coeff, c->T * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}
int hml_get_integral_array(hml_ctx* c, float* sum, float* sum_sq) {
    NEED_LOADED();
    HIPCHK(hipStreamSynchronize(c->stream));
    std::vector<float2> v(c->T + 1);
    HIPCHK(hipMemcpy(v.data(), c->d_ia, (c->T + 1) * sizeof(float2), hipMemcpyDeviceToHost));
    for (uint64_t i = 0; i <= c->T; ++i) { sum[i] = v[i].x; sum_sq[i] = v[i].y; }
    return 0;
}

// ---------------------------------------------------------------------------------------- results
int hml_recorded_sweeps(hml_ctx* c, uint64_t* n) {
    NEED_MODEL();
    hml_model m; if (int r = fetch_model(c, &m)) return r;
    *n = m.n_recorded; return 0;
}

int hml_relabel_permutation(hml_ctx* c, int32_t* perm) {
    NEED_MODEL();
    if (!perm) return set_err(HML_ERR_ARG, "null argument");
    hml_model m; if (int r = fetch_model(c, &m)) return r;
    const int K = c->K, D = m.D;
    std::vector<int32_t> p(K);
    for (int k = 0; k < K; ++k) p[k] = k;
    // ascending tuple (mean of the parameter mapped to dimension 0, dimension 1, ...); stable: ties keep their order
    std::stable_sort(p.begin(), p.end(), [&](int32_t a, int32_t b) {
        for (int d = 0; d < D; ++d) {
            const float ma = m.mu[m.map[a][d]], mb = m.mu[m.map[b][d]];
            if (ma < mb) return true;
            if (mb < ma) return false;
        }
        return false;
    });
    for (int k = 0; k < K; ++k) perm[k] = p[k];
    return 0;
}

int hml_categorical_draw(hml_ctx* c, const float* weights, int K, uint32_t* index) {
    if (!c || !weights || !index || K < 1) return set_err(HML_ERR_ARG, "invalid argument");
    // std::discrete_distribution with one weight consumes no random number and returns 0 (libstdc++)
    if (K == 1) { *index = 0; return 0; }
    const uint64_t n = c->host_draws++;
    const hml_u32x4 o = hml_stream4(hml_make_key(c->seed, c->chain), HML_KIND_HOST, n >> 32, (uint32_t)n, 0);
    *index = (uint32_t)hml_categorical(weights, K, hml_canonical_f64(o.v[0], o.v[1]));
    return 0;
}

int hml_get_stats(hml_ctx* c, hml_stats* out) {
    NEED_MODEL();
    hml_model m; if (int r = fetch_model(c, &m)) return r;
    out->sweeps = m.sweeps; out->block_updates = m.block_updates; out->uniform_fallbacks = m.uniform_fallbacks;
    out->forward_refits = m.forward_refits; out->forward_serial = m.forward_serial;
    out->forward_warmup = m.fwd_W;
    out->fused_fallbacks = m.fused_fallbacks;
    out->buffer_growths = c->grown; out->block_capacity = c->cap;
    return 0;
}

int hml_profile_enable(hml_ctx* c, int on) {
    if (!c) return set_err(HML_ERR_ARG, "null context");
    if (on && c->ev_pool.size() < 64) {
        // events for the first brackets are created here, not inside the region the caller is about to time
        // (hipEventCreate costs tens of microseconds; a 20-sweep timed region saw four of them in its first sweep)
        if (int r = ctx_bind(c)) return r;
        while (c->ev_pool.size() < 64) { hipEvent_t e; HIPCHK(hipEventCreate(&e)); c->ev_pool.push_back(e); }
    }
    c->profiling = on;
    return 0;
}

int hml_profile_get(hml_ctx* c, const char* name, double* total_ms, uint64_t* launches) {
    if (!c) return set_err(HML_ERR_ARG, "null context");
    if (int r = ctx_bind(c)) return r;
    HIPCHK(hipStreamSynchronize(c->stream));
    auto& acc = c->prof[name];
    for (auto& p : acc.pending) {
        float ms = 0;
        hipEventElapsedTime(&ms, p.first, p.second);
        acc.ms += ms; acc.n++;
        c->ev_pool.push_back(p.first); c->ev_pool.push_back(p.second);
    }
    acc.pending.clear();
    if (total_ms) *total_ms = acc.ms;
    if (launches) *launches = acc.n;
    return 0;
}

int hml_debug_eval(int device, int fn, const float* a, const float* b, float* out, uint64_t n, uint64_t seed) {
    HIPCHK(hipSetDevice(device));
    DevArr<float> d_a, d_b, d_o;
    HIPCHK(d_a.alloc(n)); HIPCHK(d_o.alloc(n));
    HIPCHK(hipMemcpy(d_a, a, n * 4, hipMemcpyHostToDevice));
    if (b) { HIPCHK(d_b.alloc(n)); HIPCHK(hipMemcpy(d_b, b, n * 4, hipMemcpyHostToDevice)); }
    hipLaunchKernelGGL(hml_k_debug_eval, dim3(1024), dim3(256), 0, 0, fn, d_a, d_b, d_o, n, seed);
    KLAUNCH_CHECK();
    HIPCHK(hipMemcpy(out, d_o, n * 4, hipMemcpyDeviceToHost));
    return 0;
}

int hml_device_memory_live(uint64_t* bytes, uint64_t* allocations) {
    if (!bytes || !allocations) return set_err(HML_ERR_ARG, "null argument");
    *bytes = hml_dev_live_bytes.load(); *allocations = hml_dev_live_allocations.load();
    return 0;
}

int hml_debug_fail_allocation(int64_t nth) {
    const int64_t made = hml_dev_alloc_seen.exchange(0);
    hml_dev_alloc_fail_at = nth > 0 ? nth : 0;
    return (int)made;
}

int hml_synth_gauss(float* x, int16_t* states, uint64_t T, int K, const float* mu, float sigma, double mean_dwell,
                    uint64_t seed, int nthreads) {
    if (!x || !mu || K < 1) return set_err(HML_ERR_ARG, "invalid argument");
    hml_synth_gauss_trace(x, states, T, K, mu, sigma, mean_dwell, seed, nthreads);
    return 0;
}


int hml_synth_depth(float* x, int16_t* states, uint64_t T, double depth, double ln_sigma, uint64_t seed, int nthreads) {
    if (!x) return set_err(HML_ERR_ARG, "invalid argument");
    hml_synth_depth_trace(x, states, T, depth, ln_sigma, seed, nthreads);
    return 0;
}

}  // extern "C"


#if defined(HML_ONLY_K)
#define HML_DECLARE_KTAB_(K) extern hml_ktab hml_ktab_##K; static const hml_ktab* ktab(int k) { return k == K ? &hml_ktab_##K : nullptr; }
#define HML_DECLARE_KTAB(K) HML_DECLARE_KTAB_(K)
HML_DECLARE_KTAB(HML_ONLY_K)
#else
#define HML_EXT_KTAB(K) extern hml_ktab hml_ktab_##K;
HML_EXT_KTAB(2) HML_EXT_KTAB(3) HML_EXT_KTAB(4) HML_EXT_KTAB(5) HML_EXT_KTAB(6) HML_EXT_KTAB(7) HML_EXT_KTAB(8) HML_EXT_KTAB(9)
HML_EXT_KTAB(10) HML_EXT_KTAB(11) HML_EXT_KTAB(12) HML_EXT_KTAB(13) HML_EXT_KTAB(14) HML_EXT_KTAB(15) HML_EXT_KTAB(16)
static const hml_ktab* ktab(int k) {
    static const hml_ktab* const tabs[17] = {nullptr, nullptr, &hml_ktab_2, &hml_ktab_3, &hml_ktab_4, &hml_ktab_5, &hml_ktab_6, &hml_ktab_7, &hml_ktab_8,
                                             &hml_ktab_9, &hml_ktab_10, &hml_ktab_11, &hml_ktab_12, &hml_ktab_13, &hml_ktab_14, &hml_ktab_15, &hml_ktab_16};
    return (k >= 2 && k <= 16) ? tabs[k] : nullptr;
}
#endif

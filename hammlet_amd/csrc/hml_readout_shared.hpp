// Host helpers of the two objects that read a chain out - hml_readout.hip (what the recorded sweeps accumulated) and hml_infer.hip
// (exact inference under the current parameters): the row scan, the model's device error, starts into lengths, and equal
// neighbours merged into runs.  Static functions and templates like the rest of hml_capi_shared.hpp: each object holds its own.
#ifndef HML_READOUT_SHARED_HPP
#define HML_READOUT_SHARED_HPP

#include "hml_capi_shared.hpp"

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

// Adjacent entries of d_key[M] with the same 16-bit key merged into runs, on stream `s`: *n_runs and, if run_len is given, the
// runs' lengths over T positions and their keys.  scatter(n_chunks, d_rc, R, d_rs, d_rq) launches the kernel that writes the R
// runs' starts d_rs and keys d_rq from the entries' starts and the exclusive run counts d_rc of the chunks of 256 entries
// (hml_k_segment.h); what else it writes per run the callable allocates, and enqueues the copy back of, itself.
template <class Scatter>
static int merge_runs(hipStream_t s, const int16_t* d_key, uint32_t M, uint32_t T, Scatter scatter, uint64_t* n_runs, uint64_t* run_len, std::vector<int16_t>& run_key) {
    const uint32_t n_chunks = (M + 255u) / 256u;
    DevBuf b_rc, b_rs, b_rq;
    HIPCHK(b_rc.alloc(((uint64_t)n_chunks + 1) * sizeof(int32_t)));
    int32_t* const d_rc = b_rc.as<int32_t>();
    HIPCHK(hipMemsetAsync(d_rc + n_chunks, 0, sizeof(int32_t), s));
    hipLaunchKernelGGL(hml_k_seg_run_count, dim3(n_chunks), dim3(256), 0, s, d_key, M, d_rc);
    hipLaunchKernelGGL(hml_k_scan_chunks<int32_t>, dim3(1), dim3(1024), 0, s, d_rc, n_chunks + 1u);   // d_rc[n_chunks] = total
    KLAUNCH_CHECK();
    int32_t R = 0;
    HIPCHK(hipMemcpyAsync(&R, d_rc + n_chunks, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    *n_runs = (uint64_t)R;
    if (!run_len) return 0;
    HIPCHK(b_rs.alloc((uint64_t)R * sizeof(uint32_t)));
    HIPCHK(b_rq.alloc((uint64_t)R * sizeof(int16_t)));
    if (int r = scatter(n_chunks, (const int32_t*)d_rc, (uint64_t)R, b_rs.as<uint32_t>(), b_rq.as<int16_t>())) return r;
    KLAUNCH_CHECK();
    std::vector<uint32_t> h_rs(R);
    run_key.resize(R);
    HIPCHK(hipMemcpyAsync(h_rs.data(), b_rs.get(), (uint64_t)R * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(run_key.data(), b_rq.get(), (uint64_t)R * sizeof(int16_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    lengths_of(h_rs.data(), (uint64_t)R, T, run_len);
    return 0;
}

#endif

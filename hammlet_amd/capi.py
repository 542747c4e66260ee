"""ctypes binding of include/hml.h (libhammlet_hip.so) - the Python-side mirror of the C ABI.

There is no CPU fallback: constructing a Chain without the compiled gfx950 library or without a
GPU raises.
"""
import ctypes as C
import os

import numpy as np

from . import build as _build

_lib = None


class HmlError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(msg)
        self.code = code


class HmlStats(C.Structure):
    _fields_ = [("sweeps", C.c_uint64), ("block_updates", C.c_uint64), ("uniform_fallbacks", C.c_uint64),
                ("forward_refits", C.c_uint64), ("forward_serial", C.c_uint64), ("forward_warmup", C.c_uint64),
                ("fused_fallbacks", C.c_uint64), ("buffer_growths", C.c_uint64), ("block_capacity", C.c_uint64)]


RECORD_CB = C.CFUNCTYPE(None, C.c_void_p, C.c_uint64, C.c_void_p)

# name -> (restype, argtypes); every symbol include/hml.h declares
_P = C.c_void_p
SIGNATURES = {
    "hml_last_error": (C.c_char_p, []),
    "hml_abi_version": (C.c_uint32, []),
    "hml_device_arch": (C.c_char_p, []),
    "hml_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "hml_create": (C.c_int, [C.POINTER(_P), C.c_int, C.c_uint64, C.c_uint32, _P]),
    "hml_destroy": (None, [_P]),
    "hml_load_observations": (C.c_int, [_P, _P, C.c_uint64]),
    "hml_load_observations_device": (C.c_int, [_P, _P, C.c_uint64]),
    "hml_attach_observations": (C.c_int, [_P, _P]),
    "hml_text_open": (C.c_int, [C.POINTER(_P), C.c_int, C.c_uint64]),
    "hml_text_close": (None, [_P]),
    "hml_text_buffer": (C.c_int, [_P, C.POINTER(_P), C.POINTER(C.c_uint64)]),
    "hml_text_commit": (C.c_int, [_P, C.c_uint64]),
    "hml_text_feed": (C.c_int, [_P, C.c_char_p, C.c_uint64]),
    "hml_text_reserve": (C.c_int, [_P, C.c_uint64]),
    "hml_text_finish": (C.c_int, [_P, C.POINTER(C.c_uint64), C.POINTER(C.c_int)]),
    "hml_text_values": (C.c_int, [_P, _P]),
    "hml_text_counters": (C.c_int, [_P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "hml_set_dimensions": (C.c_int, [_P, C.c_int, C.c_int]),
    "hml_get_dimensions": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "hml_set_weights": (C.c_int, [_P, _P, C.c_uint64]),
    "hml_noise_sigma": (C.c_int, [_P, C.POINTER(C.c_double)]),
    "hml_scale_weights": (C.c_int, [_P, C.c_float]),
    "hml_autoprior": (C.c_int, [_P, C.c_float, C.c_float, _P]),
    "hml_set_model": (C.c_int, [_P, C.c_int, _P, C.c_float, C.c_float, C.c_float, C.c_int]),
    "hml_set_self_transitions": (C.c_int, [_P, C.c_int]),
    "hml_sample_prior": (C.c_int, [_P]),
    "hml_set_static_blocks": (C.c_int, [_P]),
    "hml_set_dynamic": (C.c_int, [_P, C.c_int]),
    "hml_create_blocks": (C.c_int, [_P, C.c_float]),
    "hml_iterate": (C.c_int, [_P, C.c_char, C.c_uint64, C.c_uint64]),
    "hml_iterate_many": (C.c_int, [_P, C.c_int, C.c_char, C.c_uint64, C.c_uint64]),
    "hml_set_recording": (C.c_int, [_P, C.c_int, RECORD_CB, _P]),
    "hml_set_option": (C.c_int, [_P, C.c_char_p, C.c_int]),
    "hml_sync": (C.c_int, [_P]),
    "hml_get_num_blocks": (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    "hml_get_blocks": (C.c_int, [_P, _P]),
    "hml_get_block_stats": (C.c_int, [_P, _P, _P]),
    "hml_get_states": (C.c_int, [_P, _P]),
    "hml_get_theta": (C.c_int, [_P, _P]),
    "hml_get_transitions": (C.c_int, [_P, _P, _P]),
    "hml_set_parameters": (C.c_int, [_P, _P, _P, _P]),
    "hml_get_threshold": (C.c_int, [_P, C.POINTER(C.c_float)]),
    "hml_enable_probes": (C.c_int, [_P, C.c_int]),
    "hml_get_block_loglik": (C.c_int, [_P, _P]),
    "hml_get_forward_rows": (C.c_int, [_P, _P]),
    "hml_get_counts": (C.c_int, [_P, _P, _P, _P, _P, _P]),
    "hml_get_weights": (C.c_int, [_P, _P]),
    "hml_get_coefficients": (C.c_int, [_P, _P]),
    "hml_get_integral_array": (C.c_int, [_P, _P, _P]),
    "hml_marginals_rle": (C.c_int, [_P, C.POINTER(C.c_uint64), C.POINTER(C.c_int), _P, _P]),
    "hml_max_segmentation": (C.c_int, [_P, C.POINTER(C.c_uint64), _P, _P]),
    "hml_marginals_dense_device": (C.c_int, [_P, _P, _P]),
    "hml_recorded_sweeps": (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    "hml_set_level_recording": (C.c_int, [_P, C.c_int]),
    "hml_levels_rle": (C.c_int, [_P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), _P, _P, _P]),
    "hml_levels_dense_device": (C.c_int, [_P, _P]),
    "hml_levels_merge": (C.c_int, [_P, _P]),
    "hml_levels_on_segments": (C.c_int, [_P, C.c_uint64, _P, _P, _P]),
    "hml_levels_agreement_rle": (C.c_int, [_P, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), _P, _P, _P, _P]),
    "hml_levels_agreement_dense_device": (C.c_int, [_P, C.c_int, _P]),
    "hml_levels_agreement_summary": (C.c_int, [_P, C.c_int, C.c_double, _P, _P, _P]),
    "hml_set_break_recording": (C.c_int, [_P, C.c_int]),
    "hml_breaks_list": (C.c_int, [_P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), _P, _P]),
    "hml_breaks_dense_device": (C.c_int, [_P, _P, C.c_uint32]),
    "hml_breaks_merge": (C.c_int, [_P, _P]),
    "hml_breaks_consensus": (C.c_int, [_P, C.c_uint32, C.c_uint64, C.POINTER(C.c_uint64), _P, _P, _P]),
    "hml_set_level_bands": (C.c_int, [_P, C.c_int, _P]),
    "hml_get_level_bands": (C.c_int, [_P, C.POINTER(C.c_int), _P]),
    "hml_bands_rle": (C.c_int, [_P, C.POINTER(C.c_uint64), C.POINTER(C.c_int), C.POINTER(C.c_uint64), _P, _P]),
    "hml_bands_dense_device": (C.c_int, [_P, _P, C.c_int]),
    "hml_bands_call": (C.c_int, [_P, C.c_uint64, C.POINTER(C.c_uint64), _P, _P]),
    "hml_bands_merge": (C.c_int, [_P, _P]),
    "hml_set_regions": (C.c_int, [_P, C.c_uint64, _P, _P, C.c_int, _P]),
    "hml_get_regions": (C.c_int, [_P, C.POINTER(C.c_uint64), _P, _P, C.POINTER(C.c_int), _P]),
    "hml_regions_read": (C.c_int, [_P, C.POINTER(C.c_uint64), C.POINTER(C.c_int), C.POINTER(C.c_uint64), _P, _P, _P, _P, _P, _P]),
    "hml_regions_add": (C.c_int, [_P, C.c_uint64, _P, _P, _P, _P, _P, _P]),
    "hml_regions_merge": (C.c_int, [_P, _P]),
    "hml_set_history": (C.c_int, [_P, C.c_int, C.c_uint64]),
    "hml_history_size": (C.c_int, [_P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "hml_history_read": (C.c_int, [_P, C.c_uint64, C.c_uint64, _P]),
    "hml_history_clear": (C.c_int, [_P]),
    "hml_history_column": (C.c_char_p, [C.c_int]),
    "hml_history_stats": (C.c_int, [_P, C.c_int, C.c_uint64, C.POINTER(C.c_double), C.POINTER(C.c_double), _P, _P, C.POINTER(C.c_uint64)]),
    "hml_history_summary": (C.c_int, [_P, C.c_int, C.c_int, C.c_uint64, C.POINTER(C.c_double), C.POINTER(C.c_double), _P, _P,
                                      C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "hml_viterbi": (C.c_int, [_P, C.POINTER(C.c_uint64), _P, _P, C.POINTER(C.c_int64), C.POINTER(C.c_double)]),
    "hml_viterbi_states": (C.c_int, [_P, _P]),
    "hml_viterbi_scores": (C.c_int, [_P, _P, _P, _P]),
    "hml_viterbi_info": (C.c_int, [_P] + [C.POINTER(C.c_uint64)] * 6),
    "hml_posterior": (C.c_int, [_P, _P, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    "hml_posterior_rle": (C.c_int, [_P, C.POINTER(C.c_uint64), _P, _P, _P]),
    "hml_posterior_terms": (C.c_int, [_P, _P, _P, _P, _P, _P]),
    "hml_posterior_info": (C.c_int, [_P] + [C.POINTER(C.c_uint64)] * 7),
    "hml_expected_counts": (C.c_int, [_P] * 7 + [C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "hml_em_step": (C.c_int, [_P, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    "hml_em_fit": (C.c_int, [_P, C.c_int, C.c_uint64, C.c_double, _P, C.POINTER(C.c_uint64), C.POINTER(C.c_int), C.POINTER(C.c_uint64)]),
    "hml_em_fit_many": (C.c_int, [_P, C.c_uint64, _P, _P, _P, C.c_int, C.c_uint64, C.c_double, C.c_int] + [_P] * 8 + [C.POINTER(C.c_int64)]),
    "hml_em_starts": (C.c_int, [_P, C.c_uint64, C.c_uint64, C.c_double, _P, _P, _P]),
    "hml_em_many_info": (C.c_int, [_P] + [C.POINTER(C.c_uint64)] * 9),
    "hml_set_em_batch_bytes": (C.c_int, [_P, C.c_uint64]),
    "hml_posterior_breaks": (C.c_int, [_P, C.c_double, C.POINTER(C.c_uint64), _P, _P, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    "hml_posterior_regions": (C.c_int, [_P, C.c_uint64] + [_P] * 7 + [C.POINTER(C.c_uint64)]),
    "hml_posterior_pair_terms": (C.c_int, [_P] * 6),
    "hml_posterior_sample": (C.c_int, [_P, C.c_uint64, C.c_uint64, C.c_uint64] + [_P] * 5 + [C.POINTER(C.c_uint64)]),
    "hml_posterior_sample_regions": (C.c_int, [_P, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, _P, _P, C.c_uint32] + [_P] * 4),
    "hml_posterior_sample_info": (C.c_int, [_P] + [C.POINTER(C.c_uint64)] * 9),
    "hml_set_sample_batch_bytes": (C.c_int, [_P, C.c_uint64]),
    "hml_posterior_region_counts": (C.c_int, [_P, C.c_uint64, _P, _P, C.c_uint32, _P, _P, _P, C.POINTER(C.c_uint64)]),
    "hml_posterior_count_terms": (C.c_int, [_P, _P, _P]),
    "hml_posterior_counts_info": (C.c_int, [_P] + [C.POINTER(C.c_uint64)] * 3),
    "hml_recording_payload_size": (C.c_int, [_P, C.c_int, C.POINTER(C.c_uint64)]),
    "hml_recording_export": (C.c_int, [_P, C.c_int, _P, C.c_uint64, C.POINTER(C.c_uint64)]),
    "hml_recording_merge_payload": (C.c_int, [_P, C.c_int, _P, C.c_uint64]),
    "hml_recording_merge_across": (C.c_int, [_P, _P, C.c_int]),
    "hml_categorical_draw": (C.c_int, [_P, _P, C.c_int, C.POINTER(C.c_uint32)]),
    "hml_relabel_permutation": (C.c_int, [_P, _P]),
    "hml_pool_payload_size": (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    "hml_pool_export": (C.c_int, [_P, _P, _P]),
    "hml_pool_install": (C.c_int, [_P, _P]),
    "hml_pool_unique_id": (C.c_int, [_P]),
    "hml_pool_create": (C.c_int, [C.POINTER(_P), C.c_int, C.c_int, C.c_int, _P]),
    "hml_pool_destroy": (None, [_P]),
    "hml_pool_marginals": (C.c_int, [_P, _P, _P]),
    "hml_pool_info": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_int)]),
    "hml_pool_set_form": (C.c_int, [_P, C.c_int]),
    "hml_pool_last": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_uint64)]),
    "hml_allreduce_marginals": (C.c_int, [_P, C.c_int]),
    "hml_allreduce_marginals_perm": (C.c_int, [_P, C.c_int, _P]),
    "hml_pool_permutation": (C.c_int, [_P, _P]),
    "hml_get_stats": (C.c_int, [_P, C.POINTER(HmlStats)]),
    "hml_profile_enable": (C.c_int, [_P, C.c_int]),
    "hml_profile_get": (C.c_int, [_P, C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    "hml_debug_eval": (C.c_int, [C.c_int, C.c_int, _P, _P, _P, C.c_uint64, C.c_uint64]),
    "hml_device_memory_live": (C.c_int, [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "hml_debug_fail_allocation": (C.c_int, [C.c_int64]),
    "hml_debug_guard_allocations": (C.c_int, [C.c_uint64, C.c_int]),
    "hml_debug_check_guards": (C.c_int, [C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_int64), C.POINTER(C.c_uint64), C.POINTER(C.c_int), C.POINTER(C.c_uint64)]),
    "hml_debug_guard_selftest": (C.c_int, []),
    "hml_synth_depth": (C.c_int, [_P, _P, C.c_uint64, C.c_double, C.c_double, C.c_uint64, C.c_int]),
    "hml_synth_gauss": (C.c_int, [_P, _P, C.c_uint64, C.c_int, _P, C.c_float, C.c_double, C.c_uint64, C.c_int]),
}


ABI_VERSION = 5   # hml_abi_version() of include/hml.h this mirror was written against

# the kinds of recording of the sparse payloads (HML_RECORDING_* of include/hml.h)
RECORDING_LEVELS, RECORDING_BREAKS, RECORDING_BANDS = 0, 1, 2

# why a fit stopped (HML_EM_* of include/hml.h)
EM_MAX_STEPS, EM_CONVERGED, EM_DEGENERATE = 0, 1, 2


def load_library(path=None):
    """dlopen libhammlet_hip.so and attach the signatures of include/hml.h.  Fails loudly."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    path = path or os.environ.get("HML_LIBRARY") or _build.LIB_PATH   # HML_LIBRARY: A/B timing of two builds
    if not os.path.exists(path):
        raise HmlError(-1, "%s is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(hipcc --offload-arch=gfx950); there is no CPU fallback" % path)
    lib = C.CDLL(path, mode=C.RTLD_GLOBAL)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the library does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    if lib.hml_abi_version() != ABI_VERSION:
        raise HmlError(-1, "%s has ABI version %d, this package expects %d: rebuild the library" % (path, lib.hml_abi_version(), ABI_VERSION))
    _lib = lib
    return lib


def _check(rc):
    if rc != 0:
        raise HmlError(rc, load_library().hml_last_error().decode())


def parse_text(source, device=0, chunk_bytes=0, feed_bytes=None, with_info=False):
    """The float32 values that the reference's reader (`while ( input >> v )`, reference src/wavelet.hpp:131)
    extracts from whitespace-separated decimal text, converted on the GPU.  `source`: bytes or a file path.
    Returns the array (and, with_info, a dict: stopped, bytes, irregular_tokens, host_chunks)."""
    lib = load_library()
    h = _P()
    _check(lib.hml_text_open(C.byref(h), device, chunk_bytes))
    try:
        if isinstance(source, (bytes, bytearray, memoryview)):
            data = bytes(source)
            step = feed_bytes or max(len(data), 1)
            for i in range(0, len(data), step):
                part = data[i:i + step]
                _check(lib.hml_text_feed(h, part, len(part)))
        else:
            with open(source, "rb", buffering=0) as f:
                while True:
                    buf, cap = _P(), C.c_uint64()
                    _check(lib.hml_text_buffer(h, C.byref(buf), C.byref(cap)))
                    view = (C.c_char * cap.value).from_address(buf.value)
                    n = f.readinto(view)
                    if not n:
                        break
                    _check(lib.hml_text_commit(h, n))
        n, stopped = C.c_uint64(), C.c_int()
        _check(lib.hml_text_finish(h, C.byref(n), C.byref(stopped)))
        out = np.empty(n.value, np.float32)
        _check(lib.hml_text_values(h, out.ctypes.data))
        if not with_info:
            return out
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        _check(lib.hml_text_counters(h, C.byref(a), C.byref(b), C.byref(c)))
        return out, {"stopped": bool(stopped.value), "bytes": a.value, "irregular_tokens": b.value, "host_chunks": c.value}
    finally:
        lib.hml_text_close(h)


def synth_gauss(T, K, mu, sigma, dwell, seed, nthreads=8, with_states=False):
    lib = load_library()
    x = np.empty(T, np.float32)
    mu = np.ascontiguousarray(mu, np.float32)
    st = np.empty(T, np.int16) if with_states else None
    _check(lib.hml_synth_gauss(x.ctypes.data, st.ctypes.data if with_states else None, T, K, mu.ctypes.data, sigma,
                               dwell, seed, nthreads))
    return (x, st) if with_states else x


def synth_depth(T, depth=15.0, ln_sigma=0.15, seed=5, nthreads=8, with_states=False):
    lib = load_library()
    x = np.empty(T, np.float32)
    st = np.empty(T, np.int16) if with_states else None
    _check(lib.hml_synth_depth(x.ctypes.data, st.ctypes.data if with_states else None, T, depth, ln_sigma, seed, nthreads))
    return (x, st) if with_states else x


def debug_eval(fn, a, b=None, seed=0, device=0):
    lib = load_library()
    a = np.ascontiguousarray(a, np.float32)
    out = np.empty_like(a)
    if b is not None:
        b = np.ascontiguousarray(b, np.float32)
    _check(lib.hml_debug_eval(device, fn, a.ctypes.data, b.ctypes.data if b is not None else None, out.ctypes.data, a.size, seed))
    return out


def device_memory_live():
    """(bytes, allocations) of device memory that the library's contexts and read-outs hold now, over the whole process"""
    b, n = C.c_uint64(), C.c_uint64()
    _check(load_library().hml_device_memory_live(C.byref(b), C.byref(n)))
    return b.value, n.value


def debug_fail_allocation(nth):
    """Test hook: the nth device allocation from now (1: the next) fails once, as if out of memory; 0 turns it off.
    Returns the number of allocations made since the hook was last set."""
    return load_library().hml_debug_fail_allocation(nth)


GUARD_TAG = "hml-guard:"   # HML_GUARD_TAG: what a damaged guard's line on stderr starts with


def debug_guard_allocations(guard_bytes, poison=False):
    """Test mode: from the next device allocation on, guard bands of guard_bytes (rounded up to a multiple of 256) on both
    sides of every allocation and, with poison, a body of 0xFF bytes; 0 turns it off."""
    _check(load_library().hml_debug_guard_allocations(int(guard_bytes), 1 if poison else 0))


def debug_check_guards(reset=True):
    """Waits for the device and checks the guards of every registered allocation.  Returns a dict: damaged (allocations with a
    damaged guard since the last reset, at a check or when freed) and, of the first of them, ordinal (among the allocations
    since the mode was armed), bytes, side ("front" / "back") and offset (of the first damaged byte in that guard)."""
    n, o, b, s, at = C.c_uint64(), C.c_int64(), C.c_uint64(), C.c_int(), C.c_uint64()
    _check(load_library().hml_debug_check_guards(1 if reset else 0, C.byref(n), C.byref(o), C.byref(b), C.byref(s), C.byref(at)))
    if not n.value:
        return {"damaged": 0}
    return {"damaged": n.value, "ordinal": o.value, "bytes": b.value, "side": "back" if s.value else "front", "offset": at.value}


def debug_guard_selftest():
    """The mode's own proof that it detects (hml_debug_guard_selftest): raises HmlError if it does not, or without a GPU."""
    _check(load_library().hml_debug_guard_selftest())


class Chain:
    """One Gibbs chain on one GPU: the Python mirror of hml_ctx (see include/hml.h for the reference
    interfaces each call stands for)."""

    def __init__(self, device=0, seed=0, chain_id=0, stream=None):
        self.lib = load_library()
        h = _P()
        _check(self.lib.hml_create(C.byref(h), device, seed, chain_id, stream))
        self.h = h
        self.device = device
        self.K = None
        self.T = None
        self.D = 1          # data dimensions / emission parameters ("-s C P D"); P = None: P = K
        self.P = None
        self._cb = None

    def close(self):
        if self.h:
            self.lib.hml_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- construction -------------------------------------------------------------------
    def set_dimensions(self, D, P):
        """D data dimensions (their values follow each other in x), P emission parameters shared by P**D states"""
        _check(self.lib.hml_set_dimensions(self.h, D, P))
        self.D, self.P = D, P

    def load(self, x):
        x = np.ascontiguousarray(x, np.float32)
        self.T = int(x.size) // self.D
        _check(self.lib.hml_load_observations(self.h, x.ctypes.data, x.size))

    def load_device(self, ptr, T):
        self.T = int(T)
        _check(self.lib.hml_load_observations_device(self.h, ptr, T))

    def attach(self, source):
        """hml_attach_observations: share `source`'s construction (same device) instead of loading a copy"""
        _check(self.lib.hml_attach_observations(self.h, source.h))
        self.T, self.D, self.P = source.T, source.D, source.P

    def noise_sigma(self):
        v = C.c_double()
        _check(self.lib.hml_noise_sigma(self.h, C.byref(v)))
        return v.value

    def scale_weights(self, m):
        _check(self.lib.hml_scale_weights(self.h, m))

    def set_weights(self, w):
        w = np.ascontiguousarray(w, np.float32)
        _check(self.lib.hml_set_weights(self.h, w.ctypes.data, w.size))

    def autoprior(self, s2=0.2, p=0.9):
        out = np.empty(4, np.float32)
        _check(self.lib.hml_autoprior(self.h, s2, p, out.ctypes.data))
        return out

    def set_model(self, K, nig4, a_off=0.5, a_diag=0.5, pi_alpha=0.5, self_trans=True):
        nig4 = np.ascontiguousarray(nig4, np.float32)
        self.K = K
        _check(self.lib.hml_set_model(self.h, K, nig4.ctypes.data, a_off, a_diag, pi_alpha, 1 if self_trans else 0))

    def sample_prior(self):
        _check(self.lib.hml_sample_prior(self.h))

    def set_self_transitions(self, on=True):
        _check(self.lib.hml_set_self_transitions(self.h, 1 if on else 0))

    def set_static_blocks(self):
        _check(self.lib.hml_set_static_blocks(self.h))

    def set_dynamic(self, on=True):
        _check(self.lib.hml_set_dynamic(self.h, 1 if on else 0))

    def create_blocks(self, thr):
        _check(self.lib.hml_create_blocks(self.h, thr))

    def iterate(self, method, iterations, thinning=0):
        _check(self.lib.hml_iterate(self.h, method.encode()[0:1], iterations, thinning))

    def set_recording(self, marginals=True, callback=None):
        if callback is not None:
            def tramp(_ctx, sweep, _user):
                callback(self, sweep)
            self._cb = RECORD_CB(tramp)
        else:
            self._cb = C.cast(None, RECORD_CB)
        _check(self.lib.hml_set_recording(self.h, 1 if marginals else 0, self._cb, None))

    def set_option(self, name, value):
        _check(self.lib.hml_set_option(self.h, name.encode(), int(value)))

    def sync(self):
        _check(self.lib.hml_sync(self.h))

    # ---- probes -------------------------------------------------------------------------
    def num_blocks(self):
        v = C.c_uint64()
        _check(self.lib.hml_get_num_blocks(self.h, C.byref(v)))
        return v.value

    def blocks(self):
        B = self.num_blocks()
        s = np.empty(B + 1, np.uint32)
        _check(self.lib.hml_get_blocks(self.h, s.ctypes.data))
        return s

    def block_stats(self):
        """(sum x, sum x^2) of every block; with D > 1 data dimensions arrays of shape [D][B]"""
        B = self.num_blocks()
        a = np.empty((self.D, B), np.float32)
        b = np.empty((self.D, B), np.float32)
        _check(self.lib.hml_get_block_stats(self.h, a.ctypes.data, b.ctypes.data))
        return (a[0], b[0]) if self.D == 1 else (a, b)

    def states(self):
        B = self.num_blocks()
        q = np.empty(B, np.int16)
        _check(self.lib.hml_get_states(self.h, q.ctypes.data))
        return q

    def theta(self):
        t = np.empty(2 * (self.P or self.K), np.float32)
        _check(self.lib.hml_get_theta(self.h, t.ctypes.data))
        return t

    def transitions(self):
        A = np.empty((self.K, self.K), np.float32)
        pi = np.empty(self.K, np.float32)
        _check(self.lib.hml_get_transitions(self.h, A.ctypes.data, pi.ctypes.data))
        return A, pi

    def set_parameters(self, mean_var, A, pi):
        mv = np.ascontiguousarray(mean_var, np.float32)
        A = np.ascontiguousarray(A, np.float32)
        pi = np.ascontiguousarray(pi, np.float32)
        _check(self.lib.hml_set_parameters(self.h, mv.ctypes.data, A.ctypes.data, pi.ctypes.data))

    def threshold(self):
        v = C.c_float()
        _check(self.lib.hml_get_threshold(self.h, C.byref(v)))
        return v.value

    def enable_probes(self, on=True):
        _check(self.lib.hml_enable_probes(self.h, 1 if on else 0))

    def block_loglik(self):
        B = self.num_blocks()
        E = np.empty((B, self.K), np.float32)
        _check(self.lib.hml_get_block_loglik(self.h, E.ctypes.data))
        return E

    def forward_rows(self):
        B = self.num_blocks()
        r = np.empty((B + 1, self.K), np.float32)
        _check(self.lib.hml_get_forward_rows(self.h, r.ctypes.data))
        return r

    def counts(self):
        K = self.K
        trans = np.empty((K, K), np.uint64)
        occ = np.empty(K, np.uint64)
        s = np.empty(K, np.float32)
        q = np.empty(K, np.float32)
        n = np.empty(K, np.uint64)
        _check(self.lib.hml_get_counts(self.h, trans.ctypes.data, occ.ctypes.data, s.ctypes.data, q.ctypes.data, n.ctypes.data))
        return trans, occ, s, q, n

    def weights(self):
        w = np.empty(self.T, np.float32)
        _check(self.lib.hml_get_weights(self.h, w.ctypes.data))
        return w

    def coefficients(self):
        w = np.empty(self.T, np.float32)
        _check(self.lib.hml_get_coefficients(self.h, w.ctypes.data))
        return w

    def integral_array(self):
        a = np.empty(self.T + 1, np.float32)
        b = np.empty(self.T + 1, np.float32)
        _check(self.lib.hml_get_integral_array(self.h, a.ctypes.data, b.ctypes.data))
        return a, b

    # ---- results ------------------------------------------------------------------------
    def recorded_sweeps(self):
        v = C.c_uint64()
        _check(self.lib.hml_recorded_sweeps(self.h, C.byref(v)))
        return v.value

    def marginals_rle(self):
        n = C.c_uint64()
        k = C.c_int()
        _check(self.lib.hml_marginals_rle(self.h, C.byref(n), C.byref(k), None, None))
        seg = np.empty(n.value, np.uint64)
        cnt = np.empty((n.value, max(k.value, 0)), np.int32)
        _check(self.lib.hml_marginals_rle(self.h, C.byref(n), C.byref(k), seg.ctypes.data, cnt.ctypes.data if k.value else None))
        return seg, cnt

    def max_segmentation(self):
        """(run lengths, arg-max state per run) of the recorded marginals, merged (maxSegmentation.cpp:53-82)"""
        n = C.c_uint64()
        _check(self.lib.hml_max_segmentation(self.h, C.byref(n), None, None))
        ln = np.empty(n.value, np.uint64)
        st = np.empty(n.value, np.int32)
        _check(self.lib.hml_max_segmentation(self.h, C.byref(n), ln.ctypes.data, st.ctypes.data))
        return ln, st

    def marginals_dense_device(self, out_ptr, perm=None):
        p = None
        if perm is not None:
            perm = np.ascontiguousarray(perm, np.int32)
            p = perm.ctypes.data
        _check(self.lib.hml_marginals_dense_device(self.h, out_ptr, p))

    # ---- emission levels per position ---------------------------------------------------
    def set_level_recording(self, on=True):
        """accumulate the emission level mu(q_t) of every recorded sweep from now on (hml_set_level_recording)"""
        _check(self.lib.hml_set_level_recording(self.h, 1 if on else 0))

    def levels_rle(self):
        """(seg_len[M], n_recorded, sum[D, M], sum_sq[D, M]): the sums of the level and of its square over the recorded sweeps"""
        m, n = C.c_uint64(), C.c_uint64()
        _check(self.lib.hml_levels_rle(self.h, C.byref(m), C.byref(n), None, None, None))
        seg = np.empty(m.value, np.uint64)
        s1 = np.empty((self.D, m.value), np.float64)
        s2 = np.empty((self.D, m.value), np.float64)
        _check(self.lib.hml_levels_rle(self.h, C.byref(m), C.byref(n), seg.ctypes.data, s1.ctypes.data, s2.ctypes.data))
        return seg, n.value, s1, s2

    def levels_dense_device(self, out_ptr):
        """posterior mean (row 2 d) and standard deviation (row 2 d + 1) per position into a device buffer float32 [2 D][T]"""
        _check(self.lib.hml_levels_dense_device(self.h, out_ptr))

    def merge_levels(self, other):
        """add `other`'s recorded levels into this chain's (same GPU, positions and dimensions); no relabelling involved"""
        _check(self.lib.hml_levels_merge(self.h, other.h))

    def levels_on_segments(self, cuts):
        """(sum[D, n + 1], sum_sq[D, n + 1]): S1 and S2 of the recorded levels summed over the positions of the n + 1 segments
        that the n ascending cuts in (0, T) leave (hml_levels_on_segments); a segment's mean is sum / (N * length)"""
        cuts = np.ascontiguousarray(cuts, np.uint32)
        n = cuts.size
        s1 = np.empty((self.D, n + 1), np.float64)
        s2 = np.empty((self.D, n + 1), np.float64)
        _check(self.lib.hml_levels_on_segments(self.h, n, cuts.ctypes.data if n else None, s1.ctypes.data, s2.ctypes.data))
        return s1, s2

    # ---- breakpoint posteriors per position -----------------------------------------------
    def set_break_recording(self, on=True):
        """count the breakpoints of every recorded sweep from now on (hml_set_break_recording)"""
        _check(self.lib.hml_set_break_recording(self.h, 1 if on else 0))

    def breaks_list(self):
        """(pos[M], count[M], n_recorded): the positions where a recorded sweep changed state, ascending, and how many did"""
        m, n = C.c_uint64(), C.c_uint64()
        _check(self.lib.hml_breaks_list(self.h, C.byref(m), C.byref(n), None, None))
        pos = np.empty(m.value, np.uint32)
        cnt = np.empty(m.value, np.uint32)
        if m.value:
            _check(self.lib.hml_breaks_list(self.h, C.byref(m), C.byref(n), pos.ctypes.data, cnt.ctypes.data))
        return pos, cnt, n.value

    def breaks_dense(self, out_ptr, window=0):
        """(sum of the counts within `window` positions of t) / n_recorded per position into a device buffer float32 [T]"""
        _check(self.lib.hml_breaks_dense_device(self.h, out_ptr, window))

    def breaks_merge(self, other):
        """add `other`'s breakpoint counts into this chain's (same GPU and positions); no relabelling involved"""
        _check(self.lib.hml_breaks_merge(self.h, other.h))

    def breaks_consensus(self, window, min_count):
        """(pos[S], mass[S], peak[S]): the candidates whose windowed mass reaches min_count and that no neighbour within
        the window beats (hml_breaks_consensus), ascending"""
        s = C.c_uint64()
        _check(self.lib.hml_breaks_consensus(self.h, window, min_count, C.byref(s), None, None, None))
        pos = np.empty(s.value, np.uint32)
        mass = np.empty(s.value, np.uint64)
        peak = np.empty(s.value, np.uint32)
        if s.value:
            _check(self.lib.hml_breaks_consensus(self.h, window, min_count, C.byref(s), pos.ctypes.data, mass.ctypes.data, peak.ctypes.data))
        return pos, mass, peak

    # ---- label-free marginals: the level's posterior in bands -------------------------------
    def set_level_bands(self, edges):
        """count, per position, the recorded sweeps whose emission level falls into each of the len(edges) + 1 bands that the
        ascending `edges` define (hml_set_level_bands); an empty list turns the recording off and keeps the counts"""
        edges = np.ascontiguousarray(edges, np.float32)
        _check(self.lib.hml_set_level_bands(self.h, edges.size, edges.ctypes.data if edges.size else None))

    def level_bands(self):
        """the edges last set, float32"""
        n = C.c_int()
        edges = np.zeros(31, np.float32)
        _check(self.lib.hml_get_level_bands(self.h, C.byref(n), edges.ctypes.data))
        return edges[:n.value].copy()

    def bands_rle(self):
        """(seg_len[M], counts[M, D * (n_edges + 1)], n_recorded): per band segment, the recorded sweeps whose level lay in
        band b of dimension d, in column d * (n_edges + 1) + b"""
        m, ncol, n = C.c_uint64(), C.c_int(), C.c_uint64()
        _check(self.lib.hml_bands_rle(self.h, C.byref(m), C.byref(ncol), C.byref(n), None, None))
        seg = np.empty(m.value, np.uint64)
        cnt = np.empty((m.value, ncol.value), np.int32)
        _check(self.lib.hml_bands_rle(self.h, C.byref(m), C.byref(ncol), C.byref(n), seg.ctypes.data, cnt.ctypes.data))
        return seg, cnt, n.value

    def bands_dense_device(self, out_ptr, cumulative=False):
        """counts per position into a device buffer int32 [D * (n_edges + 1)][T]; cumulative: the sweeps in band b or above"""
        _check(self.lib.hml_bands_dense_device(self.h, out_ptr, 1 if cumulative else 0))

    def bands_call(self, rank=0):
        """(run_len[R], run_band[D, R]): the most probable band (rank 0) or the band of the rank-th smallest recorded level
        (1 <= rank <= n_recorded) per dimension, adjacent segments with the same call merged (hml_bands_call)"""
        r = C.c_uint64()
        _check(self.lib.hml_bands_call(self.h, rank, C.byref(r), None, None))
        ln = np.empty(r.value, np.uint64)
        band = np.empty((self.D, r.value), np.int32)
        _check(self.lib.hml_bands_call(self.h, rank, C.byref(r), ln.ctypes.data, band.ctypes.data))
        return ln, band

    def merge_bands(self, other):
        """add `other`'s band counts into this chain's (same GPU, positions, dimensions and edges); no relabelling involved"""
        _check(self.lib.hml_bands_merge(self.h, other.h))

    # ---- joint posteriors over caller-given regions ---------------------------------------------
    def set_regions(self, start, end, edges=()):
        """accumulate, per region [start[r], end[r]) and recorded sweep, whether the region is one segment, its number of
        breakpoints, its mean level and - with `edges` - whether all of it lies in one band (hml_set_regions); no regions
        turn the recording off and keep the regions and the sums"""
        start, end = _region_positions(start, "start"), _region_positions(end, "end")
        if start.shape != end.shape:
            raise ValueError("start and end: two one-dimensional arrays of one length")
        edges = np.ascontiguousarray(edges, np.float32)
        _check(self.lib.hml_set_regions(self.h, start.size, start.ctypes.data if start.size else None, end.ctypes.data if end.size else None,
                                        edges.size, edges.ctypes.data if edges.size else None))

    def get_regions(self):
        """(start, end, edges) last set"""
        n, ne = C.c_uint64(), C.c_int()
        _check(self.lib.hml_get_regions(self.h, C.byref(n), None, None, C.byref(ne), None))
        start, end, edges = np.empty(n.value, np.uint32), np.empty(n.value, np.uint32), np.zeros(31, np.float32)
        _check(self.lib.hml_get_regions(self.h, C.byref(n), start.ctypes.data, end.ctypes.data, C.byref(ne), edges.ctypes.data))
        return start, end, edges[:ne.value].copy()

    def regions(self):
        """the raw sums of hml_regions_read: dict(N, whole[n], breaks_sum[n], breaks_sq[n] (uint64), level_sum[D, n],
        level_sq[D, n] (float64), inband[n, D * (n_edges + 1)] (uint64; no columns without edges)); regions_summary() derives
        the probabilities, means and spreads"""
        n, ncol, N = C.c_uint64(), C.c_int(), C.c_uint64()
        _check(self.lib.hml_regions_read(self.h, C.byref(n), C.byref(ncol), C.byref(N), None, None, None, None, None, None))
        out = dict(whole=np.empty(n.value, np.uint64), breaks_sum=np.empty(n.value, np.uint64), breaks_sq=np.empty(n.value, np.uint64),
                   level_sum=np.empty((self.D, n.value), np.float64), level_sq=np.empty((self.D, n.value), np.float64),
                   inband=np.empty((n.value, ncol.value), np.uint64))
        _check(self.lib.hml_regions_read(self.h, C.byref(n), C.byref(ncol), C.byref(N), *[out[k].ctypes.data for k in REGION_SUMS]))
        out["N"] = N.value
        return out

    def regions_add(self, sums):
        """add raw sums of the same regions (a dict like regions()'s, from any chain, GPU or process) into this chain's"""
        arr = [np.ascontiguousarray(sums[k], np.float64 if k.startswith("level") else np.uint64) for k in REGION_SUMS]
        _check(self.lib.hml_regions_add(self.h, int(sums["N"]), *[a.ctypes.data if a.size else None for a in arr]))

    def regions_merge(self, other):
        """add `other`'s region sums into this chain's (same positions, dimensions, regions and edges; any two GPUs)"""
        _check(self.lib.hml_regions_merge(self.h, other.h))

    # ---- the chain's history: a row of scalars per sweep ----------------------------------------
    def set_history(self, on=True, every=1):
        """keep a row of HISTORY_COLUMNS per sweep whose number is a multiple of `every` (hml_set_history); turning it off and
        on keeps the rows"""
        _check(self.lib.hml_set_history(self.h, 1 if on else 0, int(every)))

    def _history_size(self):
        n, dropped = C.c_uint64(), C.c_uint64()
        _check(self.lib.hml_history_size(self.h, C.byref(n), C.byref(dropped)))
        return n.value, dropped.value

    def history(self):
        """the rows so far: float64 [n, 11], columns HISTORY_COLUMNS (hml_history_read)"""
        n = self._history_size()[0]
        rows = np.empty((n, HISTORY_COLS), np.float64)
        _check(self.lib.hml_history_read(self.h, 0, n, rows.ctypes.data if n else None))
        return rows

    def history_dropped(self):
        """rows that found the buffer full (0 unless something is wrong)"""
        return self._history_size()[1]

    def clear_history(self):
        _check(self.lib.hml_history_clear(self.h))

    # ---- Viterbi decode: the most probable path under the current parameters ------------------
    def viterbi(self):
        """(run_len[R], run_state[R], score): the jointly most probable state path over the current blocks under the current
        parameters, adjacent blocks of equal state merged (hml_viterbi); score = (score_fixed, score in nats)"""
        n, fixed, nats = C.c_uint64(), C.c_int64(), C.c_double()
        _check(self.lib.hml_viterbi(self.h, C.byref(n), None, None, None, None))
        ln = np.empty(n.value, np.uint64)
        st = np.empty(n.value, np.int32)
        _check(self.lib.hml_viterbi(self.h, C.byref(n), ln.ctypes.data, st.ctypes.data, C.byref(fixed), C.byref(nats)))
        return ln, st, (fixed.value, nats.value)

    def viterbi_states(self):
        """the same path per block, int16 [B] (hml_viterbi_states)"""
        q = np.empty(self.num_blocks(), np.int16)
        _check(self.lib.hml_viterbi_states(self.h, q.ctypes.data))
        return q

    def viterbi_scores(self):
        """(emit[B, K], trans[K, K], init[K]), int64 in units of 2^-20 nat: the tables a decode uses (hml_viterbi_scores)"""
        B, K = self.num_blocks(), self.K
        emit, trans, init = np.empty((B, K), np.int64), np.empty((K, K), np.int64), np.empty(K, np.int64)
        _check(self.lib.hml_viterbi_scores(self.h, emit.ctypes.data, trans.ctypes.data, init.ctypes.data))
        return emit, trans, init

    def viterbi_info(self):
        """of the last decode: dict(chunks, L, W, stale_chunks, rounds, serial_chunks) (hml_viterbi_info)"""
        v = [C.c_uint64() for _ in range(6)]
        _check(self.lib.hml_viterbi_info(self.h, *[C.byref(x) for x in v]))
        return dict(zip(("chunks", "L", "W", "stale_chunks", "rounds", "serial_chunks"), (x.value for x in v)))

    # ---- smoothing: state posteriors and log p(y | theta) under the current parameters ---------
    def posterior(self):
        """(gamma[B, K] float64, loglik, degenerate): p(q_b = j | y, theta) per block over the current blocks under the current
        parameters, the marginal log-likelihood log p(y | theta) of the compressed model, and the number of blocks no path
        reaches (hml_posterior)"""
        gamma = np.empty((self.num_blocks(), self.K), np.float64)
        loglik, degenerate = C.c_double(), C.c_uint64()
        _check(self.lib.hml_posterior(self.h, gamma.ctypes.data, C.byref(loglik), C.byref(degenerate)))
        return gamma, loglik.value, degenerate.value

    def posterior_rle(self):
        """(run_len[R], run_state[R], run_conf[R]): per block the most probable state, adjacent blocks of equal state merged,
        lengths in positions; run_conf is the smallest posterior of that state over the run's blocks (hml_posterior_rle)"""
        n, B = C.c_uint64(), self.num_blocks()      # (room for a run per block: one call, one computation)
        ln, st, cf = np.empty(B, np.uint64), np.empty(B, np.int32), np.empty(B, np.float64)
        _check(self.lib.hml_posterior_rle(self.h, C.byref(n), ln.ctypes.data, st.ctypes.data, cf.ctypes.data))
        return ln[:n.value].copy(), st[:n.value].copy(), cf[:n.value].copy()

    def posterior_terms(self):
        """(e[B, K] float32, m[B] float32, alpha[B, K], c[B], beta[B, K] float64): the tables and rows a call uses
        (hml_posterior_terms)"""
        B, K = self.num_blocks(), self.K
        e, m = np.empty((B, K), np.float32), np.empty(B, np.float32)
        alpha, c, beta = np.empty((B, K), np.float64), np.empty(B, np.float64), np.empty((B, K), np.float64)
        _check(self.lib.hml_posterior_terms(self.h, e.ctypes.data, m.ctypes.data, alpha.ctypes.data, c.ctypes.data, beta.ctypes.data))
        return e, m, alpha, c, beta

    def posterior_info(self):
        """of the last call: dict(chunks, L, W, stale_fwd, stale_bwd, rounds, serial_chunks) (hml_posterior_info)"""
        v = [C.c_uint64() for _ in range(7)]
        _check(self.lib.hml_posterior_info(self.h, *[C.byref(x) for x in v]))
        return dict(zip(("chunks", "L", "W", "stale_fwd", "stale_bwd", "rounds", "serial_chunks"), (x.value for x in v)))

    # ---- expectation-maximisation: expected counts, and a fit of theta, A and pi ----------------
    def expected_counts(self):
        """dict(xi[K, K], first[K], stay[K], occ[K], sum[K, D], sum_sq[K, D] float64, loglik, degenerate, xi_degenerate): the
        E-step over the current blocks under the current parameters; the chain is only read (hml_expected_counts)"""
        K, D = self.K, self.D
        xi, first, stay, occ = np.empty((K, K), np.float64), np.empty(K, np.float64), np.empty(K, np.float64), np.empty(K, np.float64)
        sx, sxx = np.empty((K, D), np.float64), np.empty((K, D), np.float64)
        loglik, degenerate, xi_degenerate = C.c_double(), C.c_uint64(), C.c_uint64()
        _check(self.lib.hml_expected_counts(self.h, xi.ctypes.data, first.ctypes.data, stay.ctypes.data, occ.ctypes.data, sx.ctypes.data, sxx.ctypes.data,
                                            C.byref(loglik), C.byref(degenerate), C.byref(xi_degenerate)))
        return dict(xi=xi, first=first, stay=stay, occ=occ, sum=sx, sum_sq=sxx, loglik=loglik.value, degenerate=degenerate.value,
                    xi_degenerate=xi_degenerate.value)

    def em_step(self, use_prior=False):
        """one E-step, the M-step and the installation of its result: (objective of the parameters it started from, kept)
        (hml_em_step)"""
        obj, kept = C.c_double(), C.c_uint64()
        _check(self.lib.hml_em_step(self.h, 1 if use_prior else 0, C.byref(obj), C.byref(kept)))
        return obj.value, kept.value

    def em_fit(self, max_steps, rel_tol=0.0, use_prior=False):
        """(trace[steps + 1] float64, steps, reason, kept): at most max_steps M-steps over the current blocks - which are never
        rebuilt inside a fit -, trace[k] the objective after k of them; reason is EM_MAX_STEPS, EM_CONVERGED or EM_DEGENERATE
        (hml_em_fit)"""
        trace = np.empty(int(max_steps) + 1, np.float64)
        steps, reason, kept = C.c_uint64(), C.c_int(), C.c_uint64()
        _check(self.lib.hml_em_fit(self.h, 1 if use_prior else 0, int(max_steps), float(rel_tol), trace.ctypes.data, C.byref(steps), C.byref(reason), C.byref(kept)))
        return trace[:steps.value + 1].copy(), steps.value, reason.value, kept.value

    # ---- EM from many starts ----------------------------------------------------------------------
    def em_starts(self, n, seed, spread=1.0):
        """(mean_var[n, 2 P], A[n, K, K], pi[n, K] float32): member 0 the current parameters, the others' means drawn over the
        current means' range widened by `spread` and sorted, A and pi the current ones (hml_em_starts)"""
        n, K, P = int(n), self.K, self.P or self.K
        mv, A, pi = np.empty((n, 2 * P), np.float32), np.empty((n, K, K), np.float32), np.empty((n, K), np.float32)
        _check(self.lib.hml_em_starts(self.h, n, int(seed), float(spread), mv.ctypes.data, A.ctypes.data, pi.ctypes.data))
        return mv, A, pi

    def em_fit_many(self, starts=None, n_starts=None, seed=0, spread=1.0, max_steps=30, rel_tol=0.0, use_prior=False, install=True):
        """A batch of fits, member r exactly set_parameters(start r) + em_fit(max_steps, rel_tol, use_prior): dict(trace[R,
        max_steps + 1] float64 - NaN past a member's last entry -, steps, reason, kept, mean_var[R, 2 P], A[R, K, K], pi[R, K],
        objective[R], best).  starts = (mean_var, A, pi) arrays, or n_starts members from em_starts(n_starts, seed, spread).
        install: the winner's parameters become the chain's; best = -1 (no member is a candidate) leaves them (hml_em_fit_many)"""
        K, P = self.K, self.P or self.K
        if starts is None:
            if n_starts is None:
                raise ValueError("em_fit_many: give starts or n_starts")
            starts = self.em_starts(n_starts, seed, spread)
        mv = np.ascontiguousarray(starts[0], np.float32)
        R = mv.size // (2 * P)
        A = np.ascontiguousarray(starts[1], np.float32)
        pi = np.ascontiguousarray(starts[2], np.float32)
        if mv.size != R * 2 * P or A.size != R * K * K or pi.size != R * K:
            raise ValueError("em_fit_many: starts must be mean_var[R, 2 P], A[R, K, K], pi[R, K]")
        n = int(max_steps) + 1
        trace = np.empty((R, n), np.float64)
        steps, reason, kept = np.empty(R, np.uint64), np.empty(R, np.int32), np.empty(R, np.uint64)
        fmv, fA, fpi = np.empty((R, 2 * P), np.float32), np.empty((R, K, K), np.float32), np.empty((R, K), np.float32)
        obj, best = np.empty(R, np.float64), C.c_int64()
        _check(self.lib.hml_em_fit_many(self.h, R, mv.ctypes.data, A.ctypes.data, pi.ctypes.data, 1 if use_prior else 0, int(max_steps), float(rel_tol),
                                        1 if install else 0, trace.ctypes.data, steps.ctypes.data, reason.ctypes.data, kept.ctypes.data, fmv.ctypes.data,
                                        fA.ctypes.data, fpi.ctypes.data, obj.ctypes.data, C.byref(best)))
        return dict(trace=trace, steps=steps, reason=reason, kept=kept, mean_var=fmv, A=fA, pi=fpi, objective=obj, best=best.value)

    def em_many_info(self):
        """of the last em_fit_many: dict(members, groups, group_size, esteps, launch_sets, stale_fwd, stale_bwd, rounds,
        serial_chunks) (hml_em_many_info)"""
        v = [C.c_uint64() for _ in range(9)]
        _check(self.lib.hml_em_many_info(self.h, *[C.byref(x) for x in v]))
        return dict(zip(("members", "groups", "group_size", "esteps", "launch_sets", "stale_fwd", "stale_bwd", "rounds", "serial_chunks"), (x.value for x in v)))

    def set_em_batch_bytes(self, n_bytes=0):
        """the device memory a group of em_fit_many's members may take (0: the default) (hml_set_em_batch_bytes)"""
        _check(self.lib.hml_set_em_batch_bytes(self.h, int(n_bytes)))

    # ---- pairwise read-outs of the smoothing: breakpoint and region posteriors ------------------
    def posterior_breaks(self, min_prob=0.0):
        """dict(pos[n] uint32, prob[n] float64, expected_breaks, pair_degenerate): the block boundaries whose posterior
        probability of a change of state under the current parameters is at least min_prob, by ascending position, and the
        expected number of breakpoints in the trace (hml_posterior_breaks)"""
        n, B = C.c_uint64(), self.num_blocks()      # (room for every boundary: one call, one computation)
        pos, prob = np.empty(B, np.uint32), np.empty(B, np.float64)
        total, bad = C.c_double(), C.c_uint64()
        _check(self.lib.hml_posterior_breaks(self.h, float(min_prob), C.byref(n), pos.ctypes.data, prob.ctypes.data, C.byref(total), C.byref(bad)))
        return dict(pos=pos[:n.value].copy(), prob=prob[:n.value].copy(), expected_breaks=total.value, pair_degenerate=bad.value)

    def posterior_regions(self, start, end, raw=False):
        """dict(whole[n], whole_state[n, K], expected_breaks[n], share[n, K] float64, pair_degenerate, and with raw=True
        raw[n, 2 K + 1] uint64): per region [start[r], end[r]) the probability that it holds no breakpoint, that all of it is
        in state j, the expected number of breakpoints inside it and the expected share of its positions in state j, under the
        current parameters (hml_posterior_regions); independent of set_regions()"""
        start, end = _region_positions(start, "start"), _region_positions(end, "end")
        if start.shape != end.shape:
            raise ValueError("start and end: two one-dimensional arrays of one length")
        n, K = start.size, self.K
        out = dict(whole=np.empty(n, np.float64), whole_state=np.empty((n, K), np.float64), expected_breaks=np.empty(n, np.float64),
                   share=np.empty((n, K), np.float64))
        words = np.empty((n, 2 * K + 1), np.uint64) if raw else None
        bad = C.c_uint64()
        ptr = lambda a: a.ctypes.data if a is not None and a.size else None
        _check(self.lib.hml_posterior_regions(self.h, n, ptr(start), ptr(end), ptr(out["whole"]), ptr(out["whole_state"]), ptr(out["expected_breaks"]),
                                              ptr(out["share"]), ptr(words), C.byref(bad)))
        out["pair_degenerate"] = bad.value
        if raw:
            out["raw"] = words
        return out

    def posterior_pair_terms(self):
        """dict(p[B], r[B, K] float64, pfx[B], cost[B, K], mass[B, K] uint64): the terms the two calls above are built from
        (hml_posterior_pair_terms)"""
        B, K = self.num_blocks(), self.K
        out = dict(p=np.empty(B, np.float64), r=np.empty((B, K), np.float64), pfx=np.empty(B, np.uint64), cost=np.empty((B, K), np.uint64),
                   mass=np.empty((B, K), np.uint64))
        _check(self.lib.hml_posterior_pair_terms(self.h, *[out[k].ctypes.data for k in ("p", "r", "pfx", "cost", "mass")]))
        return out

    # ---- sampled paths: independent draws from p(q | y, theta) under the current parameters ----
    def posterior_sample(self, count, seed=0, first=0, paths=False, state_counts=False):
        """dict(segments[count] uint64, score_fixed[count] int64, change_count[B] uint32, sample_degenerate, and with paths=True
        paths[count, B] uint8, with state_counts=True state_count[B, K] uint32): draws first ... first + count - 1 of whole
        state paths over the current blocks; draw r depends on (seed, r) alone (hml_posterior_sample)"""
        count, B, K = int(count), self.num_blocks(), self.K
        n = max(count, 0)
        out = dict(segments=np.empty(n, np.uint64), score_fixed=np.empty(n, np.int64), change_count=np.empty(B, np.uint32))
        q = np.empty((n, B), np.uint8) if paths else None
        sc = np.empty((B, K), np.uint32) if state_counts else None
        bad = C.c_uint64()
        ptr = lambda a: a.ctypes.data if a is not None and a.size else None
        _check(self.lib.hml_posterior_sample(self.h, int(first), count, int(seed), ptr(q), ptr(out["segments"]), ptr(out["score_fixed"]), ptr(out["change_count"]),
                                             ptr(sc), C.byref(bad)))
        out["sample_degenerate"] = bad.value
        if paths:
            out["paths"] = q
        if state_counts:
            out["state_count"] = sc
        return out

    def posterior_sample_regions(self, start, end, count, seed=0, first=0, max_breaks=8):
        """dict(hist[n, max_breaks + 1], whole_state[n, K] uint32, breaks_sum[n], breaks_sq[n] uint64): per region [start[r],
        end[r]) over the draws first ... first + count - 1 the histogram of the number of breakpoints inside it (last bin: that
        many or more), the draws with none and all of it in state j, and the sum and sum of squares of that number
        (hml_posterior_sample_regions)"""
        start, end = _region_positions(start, "start"), _region_positions(end, "end")
        if start.shape != end.shape:
            raise ValueError("start and end: two one-dimensional arrays of one length")
        n, K, H = start.size, self.K, int(max_breaks)
        out = dict(hist=np.zeros((n, max(H, 0) + 1), np.uint32), whole_state=np.zeros((n, K), np.uint32), breaks_sum=np.zeros(n, np.uint64),
                   breaks_sq=np.zeros(n, np.uint64))
        ptr = lambda a: a.ctypes.data if a is not None and a.size else None
        _check(self.lib.hml_posterior_sample_regions(self.h, int(first), int(count), int(seed), n, ptr(start), ptr(end), H, ptr(out["hist"]), ptr(out["whole_state"]),
                                                     ptr(out["breaks_sum"]), ptr(out["breaks_sq"])))
        return out

    def posterior_sample_info(self):
        """of the last posterior_sample / posterior_sample_regions: dict(draws, groups, group_size, chunks, L, W, stale_first,
        rounds, serial_chunks) (hml_posterior_sample_info)"""
        v = [C.c_uint64() for _ in range(9)]
        _check(self.lib.hml_posterior_sample_info(self.h, *[C.byref(x) for x in v]))
        return dict(zip(("draws", "groups", "group_size", "chunks", "L", "W", "stale_first", "rounds", "serial_chunks"), (x.value for x in v)))

    def set_sample_batch_bytes(self, n_bytes=0):
        """the device memory a group of posterior_sample's draws may take (0: the default) (hml_set_sample_batch_bytes)"""
        _check(self.lib.hml_set_sample_batch_bytes(self.h, int(n_bytes)))

    # ---- count read-outs of the smoothing: exact breakpoint-count and state-avoidance posteriors ----
    def posterior_region_counts(self, start, end, max_breaks=8):
        """dict(hist[n, max_breaks + 1], whole_state[n, K], avoid[n, K] float64, count_degenerate): per region [start[r],
        end[r]) the exact posterior distribution of the number of breakpoints inside it (last bin: that many or more), the
        probability that all of it is in state j, and the probability that no position of it is in state j, under the current
        parameters (hml_posterior_region_counts); independent of set_regions()"""
        start, end = _region_positions(start, "start"), _region_positions(end, "end")
        if start.shape != end.shape:
            raise ValueError("start and end: two one-dimensional arrays of one length")
        n, K, H = start.size, self.K, int(max_breaks)
        if not 0 <= H < 2 ** 32:
            raise ValueError("max_breaks: an unsigned 32-bit number")
        out = dict(hist=np.zeros((n, min(H, 32) + 1), np.float64), whole_state=np.zeros((n, K), np.float64), avoid=np.zeros((n, K), np.float64))
        bad = C.c_uint64()
        ptr = lambda a: a.ctypes.data if a is not None and a.size else None
        _check(self.lib.hml_posterior_region_counts(self.h, n, ptr(start), ptr(end), H, ptr(out["hist"]), ptr(out["whole_state"]), ptr(out["avoid"]), C.byref(bad)))
        out["count_degenerate"] = bad.value
        return out

    def posterior_count_terms(self):
        """dict(v[B, K], rho[B, K] float64): the terms the call above is built from (hml_posterior_count_terms)"""
        B, K = self.num_blocks(), self.K
        out = dict(v=np.empty((B, K), np.float64), rho=np.empty((B, K), np.float64))
        _check(self.lib.hml_posterior_count_terms(self.h, out["v"].ctypes.data, out["rho"].ctypes.data))
        return out

    def posterior_counts_info(self):
        """of the last posterior_region_counts: dict(regions, steps, longest) - steps the sum over the regions of the blocks a
        walk steps over (be - ba), longest the largest (hml_posterior_counts_info)"""
        v = [C.c_uint64() for _ in range(3)]
        _check(self.lib.hml_posterior_counts_info(self.h, *[C.byref(x) for x in v]))
        return dict(zip(("regions", "steps", "longest"), (x.value for x in v)))

    # ---- sparse payloads of the levels, breakpoints and bands (across GPUs) -------------------
    def recording_payload_size(self, kind):
        """bytes of the payload hml_recording_export would write now for RECORDING_LEVELS / _BREAKS / _BANDS"""
        n = C.c_uint64()
        _check(self.lib.hml_recording_payload_size(self.h, kind, C.byref(n)))
        return n.value

    def recording_export(self, kind, payload_ptr, capacity_bytes):
        """the recording's positions and raw cells into a device buffer of this chain's GPU (layout: include/hml.h); returns
        the bytes written"""
        n = C.c_uint64()
        _check(self.lib.hml_recording_export(self.h, kind, payload_ptr, capacity_bytes, C.byref(n)))
        return n.value

    def recording_merge_payload(self, kind, payload_ptr, n_bytes):
        """add a payload that lies on this chain's GPU into its recording, as merge_levels / breaks_merge / merge_bands add the
        exporting chain; checked before anything is written"""
        _check(self.lib.hml_recording_merge_payload(self.h, kind, payload_ptr, n_bytes))

    def recording_merge_across(self, other, kind):
        """add `other`'s recording into this chain's through the payload: `other` may live on another GPU"""
        _check(self.lib.hml_recording_merge_across(self.h, other.h, kind))

    # ---- chain-parallel pooling ---------------------------------------------------------
    def relabel_permutation(self):
        perm = np.empty(self.K, np.int32)
        _check(self.lib.hml_relabel_permutation(self.h, perm.ctypes.data))
        return perm

    def pool_payload_size(self):
        n = C.c_uint64()
        _check(self.lib.hml_pool_payload_size(self.h, C.byref(n)))
        return n.value

    def pool_export(self, payload_ptr):
        perm = np.empty(self.K, np.int32)
        _check(self.lib.hml_pool_export(self.h, payload_ptr, perm.ctypes.data))
        return perm

    def pool_permutation(self):
        """perm[j] = this chain's label of pooled state j (identity before any pooling)"""
        perm = np.zeros(self.K, np.int32)
        _check(self.lib.hml_pool_permutation(self.h, perm.ctypes.data))
        return perm

    def pool_install(self, payload_ptr):
        _check(self.lib.hml_pool_install(self.h, payload_ptr))

    def categorical_draw(self, weights):
        w = np.ascontiguousarray(weights, np.float32)
        out = C.c_uint32()
        _check(self.lib.hml_categorical_draw(self.h, w.ctypes.data, w.size, C.byref(out)))
        return out.value

    def stats(self):
        s = HmlStats()
        _check(self.lib.hml_get_stats(self.h, C.byref(s)))
        return {f: getattr(s, f) for f, _ in HmlStats._fields_}

    def profile_enable(self, level=2):
        _check(self.lib.hml_profile_enable(self.h, int(level)))

    def profile_get(self, name):
        ms = C.c_double()
        n = C.c_uint64()
        _check(self.lib.hml_profile_get(self.h, name.encode(), C.byref(ms), C.byref(n)))
        return ms.value, n.value


def _prefer_torch_rccl():
    """A Python process that also runs PyTorch must not hold two RCCL libraries (torch bundles one; the second copy ends the
    process in `double free or corruption` at exit): point the library's dlopen at torch's copy before its first pooling
    call, without importing torch.  No torch, or HML_RCCL_LIBRARY set by the user: nothing happens."""
    if os.environ.get("HML_RCCL_LIBRARY"):
        return
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
        cand = os.path.join(os.path.dirname(spec.origin), "lib", "librccl.so") if spec and spec.origin else None
        if cand and os.path.exists(cand):
            os.environ["HML_RCCL_LIBRARY"] = cand
            # ... and let torch bring up its runtime FIRST: an RCCL communicator created before `import torch` has been seen
            # to end the process in the same way when it exits (the order of the two libraries' exit handlers)
            import torch  # noqa: F401
    except Exception:
        pass


class Pool:
    """RCCL communicator of the chain-parallel pooling (hml_pool_* of include/hml.h): one rank per process and GPU."""

    def __init__(self, device, rank, n_ranks, unique_id):
        _prefer_torch_rccl()
        self.lib = load_library()
        h = _P()
        buf = C.create_string_buffer(bytes(unique_id), 128)
        _check(self.lib.hml_pool_create(C.byref(h), device, rank, n_ranks, C.cast(buf, _P)))
        self.h = h

    @staticmethod
    def unique_id():
        """ncclGetUniqueId: made by rank 0, handed to every rank by the launcher"""
        _prefer_torch_rccl()
        lib = load_library()
        buf = C.create_string_buffer(128)
        _check(lib.hml_pool_unique_id(C.cast(buf, _P)))
        return buf.raw

    def marginals(self, chain):
        """export + ncclAllReduce(sum, int32) + install: afterwards `chain` holds the pooled marginals"""
        perm = np.empty(chain.K, np.int32)
        _check(self.lib.hml_pool_marginals(self.h, chain.h, perm.ctypes.data))
        return perm

    def info(self):
        r, n, ms, b, v = C.c_int(), C.c_int(), C.c_double(), C.c_uint64(), C.c_int()
        _check(self.lib.hml_pool_info(self.h, C.byref(r), C.byref(n), C.byref(ms), C.byref(b), C.byref(v)))
        return {"rank": r.value, "n_ranks": n.value, "last_allreduce_ms": ms.value, "last_bytes": b.value, "rccl_version": v.value}

    def set_form(self, form):
        """0: dense payload or boundary lists, whichever is smaller (default); 1: dense (ncclAllReduce); 2: lists (ncclAllGather)"""
        _check(self.lib.hml_pool_set_form(self.h, form))

    def last(self):
        f, e = C.c_int(), C.c_uint64()
        _check(self.lib.hml_pool_last(self.h, C.byref(f), C.byref(e)))
        return {"form": {1: "dense", 2: "lists"}.get(f.value, "none"), "entries": e.value}

    def close(self):
        if self.h:
            self.lib.hml_pool_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def allreduce_marginals(chains, with_perms=False):
    """hml_allreduce_marginals(_perm): one process driving several chains (possibly on several GPUs).  with_perms: returns
    perms[i][j] = chain i's own label of pooled state j."""
    _prefer_torch_rccl()
    lib = load_library()
    arr = (_P * len(chains))(*[c.h for c in chains])
    if not with_perms:
        _check(lib.hml_allreduce_marginals(C.cast(arr, _P), len(chains)))
        return None
    perms = np.zeros((len(chains), chains[0].K), np.int32)
    _check(lib.hml_allreduce_marginals_perm(C.cast(arr, _P), len(chains), perms.ctypes.data))
    return perms


def iterate_many(chains, method, iterations, thinning=0):
    """hml_iterate_many: `iterations` sweeps of every chain; chains of one GPU and one shape share their launches"""
    lib = load_library()
    arr = (_P * len(chains))(*[c.h for c in chains])
    _check(lib.hml_iterate_many(C.cast(arr, _P), len(chains), method.encode(), iterations, thinning))


def _handles(chains):
    return C.cast((_P * len(chains))(*[c.h for c in chains]), _P)


# ---- the chains' history (hml_set_history ... hml_history_summary of include/hml.h) ----
HISTORY_COLS = 11
HISTORY_COLUMNS = ("sweep", "method", "ll_emit", "ll_path", "lprior_theta", "lprior_path", "segments", "blocks", "states_used",
                   "threshold", "chain")
HISTORY_LOGLIK, HISTORY_LOGPOST = 100, 101      # ll_emit + ll_path; ... + lprior_theta + lprior_path


def history_column(col):
    """the name of column `col` (hml_history_column); None beyond the last"""
    s = load_library().hml_history_column(int(col))
    return s.decode() if s is not None else None


def _history_result(n_chains, call):
    rhat, ess, bad = C.c_double(), C.c_double(), C.c_uint64()
    mean, sd = np.empty(n_chains, np.float64), np.empty(n_chains, np.float64)
    extra = call(C.byref(rhat), C.byref(ess), mean.ctypes.data, sd.ctypes.data, C.byref(bad))
    return dict(extra or {}, rhat=rhat.value, ess=ess.value, chain_mean=mean, chain_sd=sd, n_nonfinite=bad.value)


def history_stats(x):
    """split R-hat and effective sample size of one scalar over chains (hml_history_stats): x float64 [n_chains, n] (or [n]:
    one chain) -> dict(rhat, ess, chain_mean[n_chains], chain_sd[n_chains], n_nonfinite)"""
    x = np.ascontiguousarray(np.atleast_2d(np.asarray(x, np.float64)))
    lib = load_library()

    def call(rhat, ess, mean, sd, bad):
        _check(lib.hml_history_stats(x.ctypes.data, x.shape[0], x.shape[1], rhat, ess, mean, sd, bad))
    return _history_result(x.shape[0], call)


def history_summary(chains, col, skip_sweeps=0):
    """hml_history_stats of column `col` (an index, a name of HISTORY_COLUMNS, "loglik" or "logpost") of the chains' histories
    (hml_history_summary): the rows with sweep <= skip_sweeps are left out, the last n_used rows of every chain are used"""
    if isinstance(col, str):
        col = {"loglik": HISTORY_LOGLIK, "logpost": HISTORY_LOGPOST}.get(col, HISTORY_COLUMNS.index(col) if col in HISTORY_COLUMNS else -1)
    lib = load_library()
    used = C.c_uint64()

    def call(rhat, ess, mean, sd, bad):
        _check(lib.hml_history_summary(_handles(chains), len(chains), int(col), int(skip_sweeps), rhat, ess, mean, sd, C.byref(used), bad))
        return dict(n_used=used.value)
    return _history_result(len(chains), call)


def levels_agreement_rle(chains):
    """(seg_len[U], n_recorded, within[D, U], between[D, U], rhat[D, U]): the Gelman-Rubin R-hat of the emission level over
    the chains, per segment of the union of their level boundaries (hml_levels_agreement_rle); the chains are only read"""
    lib = load_library()
    arr = _handles(chains)
    u, n = C.c_uint64(), C.c_uint64()
    _check(lib.hml_levels_agreement_rle(arr, len(chains), C.byref(u), C.byref(n), None, None, None, None))
    D = chains[0].D
    seg = np.empty(u.value, np.uint64)
    within = np.empty((D, u.value), np.float64)
    between = np.empty((D, u.value), np.float64)
    rhat = np.empty((D, u.value), np.float64)
    _check(lib.hml_levels_agreement_rle(arr, len(chains), C.byref(u), C.byref(n), seg.ctypes.data, within.ctypes.data,
                                        between.ctypes.data, rhat.ctypes.data))
    return seg, n.value, within, between, rhat


def levels_agreement_dense_device(chains, out_ptr):
    """R-hat per position into a device buffer float32 [D][T] (hml_levels_agreement_dense_device)"""
    _check(load_library().hml_levels_agreement_dense_device(_handles(chains), len(chains), out_ptr))


def levels_agreement_summary(chains, threshold):
    """(n_above[D], max_finite[D], n_infinite[D]): the positions with R-hat above `threshold` (+inf included), the largest
    finite R-hat (0 if none) and the positions with R-hat == +inf, per dimension (hml_levels_agreement_summary)"""
    D = chains[0].D
    above = np.zeros(D, np.uint64)
    largest = np.zeros(D, np.float64)
    infinite = np.zeros(D, np.uint64)
    _check(load_library().hml_levels_agreement_summary(_handles(chains), len(chains), float(threshold), above.ctypes.data,
                                                       largest.ctypes.data, infinite.ctypes.data))
    return above, largest, infinite


def levels_rhat(n_recorded, s1, s2):
    """(within, between, rhat), float64 of shape s1.shape[1:]: the formula of hml_levels_agreement_rle (include/hml.h) in
    numpy, in the same order of operations.  s1, s2: [n][D][U], the chains' S1 and S2 per union segment; n_recorded = N >= 2."""
    s1 = np.asarray(s1, np.float64)
    s2 = np.asarray(s2, np.float64)
    n = s1.shape[0]
    N = np.float64(n_recorded)
    sq = np.zeros(s1.shape[1:], np.float64)
    sm = np.zeros(s1.shape[1:], np.float64)
    means = []
    for c in range(n):   # (from chain 0 upward, starting at 0.0)
        m = s1[c] / N
        q = s2[c] / N - m * m
        q = np.where(q > 0.0, q, 0.0)
        sq = sq + q
        sm = sm + m
        means.append(m)
    w0 = sq / np.float64(n)
    mbar = sm / np.float64(n)
    sb = np.zeros(s1.shape[1:], np.float64)
    for m in means:
        sb = sb + (m - mbar) * (m - mbar)
    between = sb / (np.float64(n) - 1.0)
    within = w0 * (N / (N - 1.0))
    with np.errstate(divide="ignore", invalid="ignore"):
        rhat = np.where(within > 0.0, np.sqrt((w0 + between) / within), np.where(between == 0.0, 1.0, np.inf))
    return within, between, rhat


def levels_mean_sd(n, s1, s2):
    """Posterior mean and standard deviation of the level from Chain.levels_rle()'s sums, as float32: S1 / N and
    sqrt(max(0, S2 / N - (S1 / N)^2)) in double, rounded once - the formula of hml_levels_dense_device.  n = 0: NaN."""
    s1 = np.asarray(s1, np.float64)
    s2 = np.asarray(s2, np.float64)
    if n == 0:
        nan = np.full(s1.shape, np.nan, np.float32)
        return nan, nan.copy()
    mean = s1 / np.float64(n)
    var = s2 / np.float64(n) - mean * mean
    return mean.astype(np.float32), np.sqrt(np.maximum(var, 0.0)).astype(np.float32)


def _region_positions(values, name):
    """positions as uint32, refused - not wrapped - when they are negative, not whole or beyond 2^32 - 1"""
    a = np.asarray(values)
    if a.ndim != 1:
        raise ValueError("%s: a one-dimensional array of positions" % name)
    if a.size == 0:
        return np.zeros(0, np.uint32)
    if a.dtype.kind not in "iu":
        if a.dtype.kind != "f" or not np.all(np.isfinite(a)) or np.any(a != np.floor(a)):
            raise ValueError("%s: positions are whole numbers" % name)
    if np.any(a < 0) or np.any(a > 2 ** 32 - 1):
        raise ValueError("%s: positions lie in [0, 2^32 - 1]" % name)
    return np.ascontiguousarray(a.astype(np.uint64), np.uint32)


REGION_SUMS = ("whole", "breaks_sum", "breaks_sq", "level_sum", "level_sq", "inband")   # the arrays of hml_regions_read, in its order
U64_MAX = 2 ** 64 - 1


def regions_summary(sums):
    """What a caller wants of Chain.regions()'s raw sums, in double: p_whole[n] = whole / N; breaks_mean[n] and breaks_sd[n] of the
    number of breakpoints inside the region (sd: not a number where breaks_sq is saturated at 2^64 - 1); level_mean[D, n] and
    level_sd[D, n] of the region's mean level; p_inband[n, columns] = inband / N.  sd = sqrt(max(0, S2 / N - (S1 / N)^2)).
    N = 0: everything not a number."""
    N = int(sums["N"])
    whole, bsum, bsq = (np.asarray(sums[k], np.uint64) for k in REGION_SUMS[:3])
    lsum, lsq = np.asarray(sums["level_sum"], np.float64), np.asarray(sums["level_sq"], np.float64)
    inband = np.asarray(sums["inband"], np.uint64)
    if N == 0:
        nan = lambda a: np.full(a.shape, np.nan, np.float64)
        return dict(N=0, p_whole=nan(whole), breaks_mean=nan(bsum), breaks_sd=nan(bsq), level_mean=nan(lsum), level_sd=nan(lsq), p_inband=nan(inband))
    n = np.float64(N)
    bmean = bsum.astype(np.float64) / n
    bsd = np.sqrt(np.maximum(bsq.astype(np.float64) / n - bmean * bmean, 0.0))
    bsd[bsq == np.uint64(U64_MAX)] = np.nan
    lmean = lsum / n
    with np.errstate(invalid="ignore"):
        lsd = np.sqrt(np.maximum(lsq / n - lmean * lmean, 0.0))
    return dict(N=N, p_whole=whole.astype(np.float64) / n, breaks_mean=bmean, breaks_sd=bsd, level_mean=lmean, level_sd=lsd,
                p_inband=inband.astype(np.float64) / n)


def bands_exceedance(counts, n_edges, D):
    """Per-edge exceedance counts from Chain.bands_rle()'s counts [M, D * (n_edges + 1)]: out[i, d * n_edges + j] = the
    recorded sweeps whose level of dimension d on segment i was >= edges[j] (the sum of the bands above the edge), int64."""
    counts = np.asarray(counts, np.int64)
    nb = n_edges + 1
    per_dim = counts.reshape(counts.shape[0], D, nb)
    above = np.cumsum(per_dim[:, :, ::-1], axis=2)[:, :, ::-1]   # [.., b] = the bands b and above
    return np.ascontiguousarray(above[:, :, 1:]).reshape(counts.shape[0], D * n_edges)


def marginals_text(seg, cnt):
    """StateMarginals::save format (reference src/StateMarginals.hpp:268-310)."""
    lines = []
    for i in range(len(seg)):
        lines.append("\t".join([str(int(seg[i]))] + [str(int(v)) for v in cnt[i]]))
    return "\n".join(lines) + "\n"

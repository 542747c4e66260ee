"""hammlet_amd - MI355X-native Forward-Backward Gibbs sampling over wavelet-compressed blocks.

The product is the gfx950 shared library behind include/hml.h (hammlet_amd/csrc) and the `hammlet`
command-line driver; this package is the thin Python mirror of that C ABI used by the tests, the
benchmark and the multi-GPU chain pooling.
"""
from .capi import allreduce_marginals, bands_exceedance, iterate_many, Chain, debug_eval, debug_check_guards, debug_fail_allocation, debug_guard_allocations, debug_guard_selftest, device_memory_live, GUARD_TAG, Pool, HmlError, history_column, history_stats, history_summary, HISTORY_COLS, HISTORY_COLUMNS, HISTORY_LOGLIK, HISTORY_LOGPOST, levels_agreement_dense_device, levels_agreement_rle, levels_agreement_summary, levels_mean_sd, levels_rhat, load_library, marginals_text, parse_text, regions_summary, synth_depth, synth_gauss, RECORDING_LEVELS, RECORDING_BREAKS, RECORDING_BANDS, EM_MAX_STEPS, EM_CONVERGED, EM_DEGENERATE  # noqa: F401
from . import build  # noqa: F401

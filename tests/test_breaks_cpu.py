"""Breakpoint posteriors and the consensus segmentation (include/hml.h: hml_set_break_recording, hml_breaks_list,
hml_breaks_dense_device, hml_breaks_merge, hml_breaks_consensus, hml_levels_on_segments) - what can be checked without a
GPU: the library's surface, the numpy restatement of tests/breaks_util.py on the CPU checker's chains, and that every
consensus case of tests/test_gpu_breaks.py (tests/breaks_cases.py) is non-vacuous on the checker's own chain."""
import ctypes

import numpy as np
import pytest

from tests import breaks_cases as bc
from tests import breaks_util as bu
from tests import levels_util as lu

CALLS = ("hml_set_break_recording", "hml_breaks_list", "hml_breaks_dense_device", "hml_breaks_merge", "hml_breaks_consensus",
         "hml_levels_on_segments")


def test_library_exports_the_break_calls():
    from hammlet_amd import build, capi
    build.build_library()
    lib = ctypes.CDLL(build.LIB_PATH)
    for name in CALLS:
        assert hasattr(lib, name), name
        assert name in capi.SIGNATURES
    lib.hml_abi_version.restype = ctypes.c_uint32
    assert lib.hml_abi_version() == 5
    assert capi.ABI_VERSION == 5
    for name in ("set_break_recording", "breaks_list", "breaks_dense", "breaks_merge", "breaks_consensus", "levels_on_segments"):
        assert hasattr(capi.Chain, name)


def _sweeps(name):
    c = bc.CASES[name]
    o = bc.checker(name)
    try:
        return bc.checker_sweeps(o, c["scheme"])
    finally:
        o.close()


_cache = {}


def sweeps_of(name):
    if name not in _cache:
        _cache[name] = _sweeps(name)
    return _cache[name]


@pytest.mark.parametrize("name", sorted(bc.CASES))
def test_counts_are_the_changes_of_state(name):
    """sum_t C[t] = the number of adjacent block pairs with different states over the recorded sweeps; position 0 never
    counts; the listed positions are a subset of the levels' boundaries"""
    c = bc.CASES[name]
    sweeps = sweeps_of(name)
    C, N = bu.counts(sweeps, c["T"])
    changes = sum(int(np.sum(np.asarray(st[1:]) != np.asarray(st[:-1]))) for _, st, _ in sweeps)
    assert int(C.sum()) == changes and changes > 0
    assert C[0] == 0 and N == len(sweeps) and C.max() <= N
    boundary = lu.accumulate(sweeps, c["T"], D=c["D"], P=c["P"] or c["K"])[2]
    pos, cnt = bu.listing(C)
    assert np.all(boundary[pos]) and int(boundary.sum()) == len(pos) + 1   # (the levels add position 0)


@pytest.mark.parametrize("name", ["k2", "k4_mixed"])
def test_merge_of_two_halves_is_the_whole(name):
    c = bc.CASES[name]
    sweeps = sweeps_of(name)
    h = len(sweeps) // 2
    Ca, Na = bu.counts(sweeps[:h], c["T"])
    Cb, Nb = bu.counts(sweeps[h:], c["T"])
    C, N = bu.counts(sweeps, c["T"])
    assert np.array_equal(Ca + Cb, C) and Na + Nb == N
    for w in bc.DENSE_WINDOWS:
        assert np.array_equal(bu.windowed(Ca, w) + bu.windowed(Cb, w), bu.windowed(C, w))


def test_helper_by_hand():
    """three sweeps on ten positions"""
    sweeps = [(np.array([0, 3, 5, 10]), np.array([0, 1, 1]), None),      # break at 3 (the block at 5 keeps the state)
              (np.array([0, 3, 4, 10]), np.array([2, 0, 2]), None),      # breaks at 3 and 4
              (np.array([0, 8, 10]), np.array([1, 0]), None)]            # break at 8
    C, N = bu.counts(sweeps, 10)
    assert N == 3 and list(C) == [0, 0, 0, 2, 1, 0, 0, 0, 1, 0]
    assert list(bu.windowed(C, 1)) == [0, 0, 2, 3, 3, 1, 0, 1, 1, 1]
    assert np.array_equal(bu.dense(C, N, 0), (C / 3.0).astype(np.float32))
    assert np.all(np.isnan(bu.dense(C, 0, 0)))
    (pos, mass, peak), (mass_all, beaten) = bu.consensus(C, 1, 2)
    # candidates 3 (C 2), 4 (C 1, beaten by 3), 8 (C 1, mass 1 < 2)
    assert list(pos) == [3] and list(mass) == [3] and list(peak) == [2]
    assert list(mass_all) == [3, 3, 1] and list(beaten) == [False, True, False]
    # equal counts: the lower position wins, and whether the winner is selected itself plays no part
    C2 = np.array([0, 1, 1, 1, 0, 0])
    (pos, mass, peak), _ = bu.consensus(C2, 1, 1)
    assert list(pos) == [1]
    (pos, _, _), _ = bu.consensus(C2, 1, 3)
    assert list(pos) == []                        # 1 has mass 2 < 3; 2 (mass 3) is beaten by 1 all the same
    assert bu.min_count_of(0.5, 15) == 8 and bu.min_count_of(0.0, 15) == 1 and bu.min_count_of(1.0, 12) == 12
    sums, length = bu.segment_sums(np.array([[1.0, 2.0, 3.0, 4.0]]), [1, 3])
    assert list(sums[0]) == [1.0, 5.0, 4.0] and list(length) == [1, 2, 1]


@pytest.mark.parametrize("window,P", bc.CONSENSUS)
@pytest.mark.parametrize("name", sorted(bc.CASES))
def test_consensus_cases_are_not_vacuous(name, window, P):
    """every (trace, window, min_count) of the GPU tests, on the checker's chain: a selected candidate, one suppressed by a
    neighbour although its mass suffices, one below min_count - and a cut of the levels_on_segments test that falls strictly
    inside a fine level segment"""
    c = bc.CASES[name]
    sweeps = sweeps_of(name)
    C, N = bu.counts(sweeps, c["T"])
    prof = bu.consensus_profile(C, window, bu.min_count_of(P, N))
    assert prof["selected"] >= 1 and prof["suppressed"] >= 1 and prof["below"] >= 1, prof
    boundary = lu.accumulate(sweeps, c["T"], D=c["D"], P=c["P"] or c["K"])[2]
    cuts = bc.arbitrary_cuts(c["T"])
    assert len(cuts) >= 30 and bu.cuts_inside_fine_segments(boundary, cuts) >= 1
    # the consensus cuts themselves are level boundaries: the union with the arbitrary ones is what splits fine segments
    (pos, _, _), _ = bu.consensus(C, window, bu.min_count_of(P, N))
    assert bu.cuts_inside_fine_segments(boundary, pos) == 0

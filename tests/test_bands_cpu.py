"""Level bands per position (include/hml.h: hml_set_level_bands, hml_get_level_bands, hml_bands_rle, hml_bands_dense_device,
hml_bands_call, hml_bands_merge) - what can be checked without a GPU: the library's surface, the numpy restatement of
tests/bands_util.py by hand and against the CPU checker's own marginals, and that every case of tests/test_gpu_bands.py has
something to find (tests/bands_cases.py)."""
import ctypes
import math

import numpy as np
import pytest

from tests import bands_cases as bc
from tests import bands_util as bu
from tests import levels_util as lu
from tests import oracle_lib as ol

CALLS = ("hml_set_level_bands", "hml_get_level_bands", "hml_bands_rle", "hml_bands_dense_device", "hml_bands_call", "hml_bands_merge")


def test_library_exports_the_band_calls():
    from hammlet_amd import build, capi
    build.build_library()
    lib = ctypes.CDLL(build.LIB_PATH)
    for name in CALLS:
        assert hasattr(lib, name), name
        assert name in capi.SIGNATURES
    lib.hml_abi_version.restype = ctypes.c_uint32
    assert lib.hml_abi_version() == 5 and capi.ABI_VERSION == 5      # additions only
    for name in ("set_level_bands", "level_bands", "bands_rle", "bands_dense_device", "bands_call", "merge_bands"):
        assert hasattr(capi.Chain, name)
    assert callable(capi.bands_exceedance)


def test_helper_bands_by_hand():
    """six positions, two sweeps, D = 2 over P = 2 parameters, one edge at 1.0.  Sweep 0: the parameter means are 1.0 - exactly
    on the edge, so band 1 - and -2.0 (band 0).  Sweep 1: both parameters lie in band 0 (0.5 and -3.0), so its two different
    states 1 and 2 share every band and cut nothing."""
    edges = [1.0]
    sweeps = [(np.array([0, 2, 4, 6]), np.array([0, 0, 3]), np.array([1.0, -2.0], np.float32)),
              (np.array([0, 3, 6]), np.array([1, 2]), np.array([0.5, -3.0], np.float32))]
    assert list(bu.band_of(edges, [1.0, np.nextafter(np.float32(1.0), np.float32(0.0)), -2.0, np.nan])) == [1, 0, 0, 0]
    counts, boundary, N = bu.accumulate(sweeps, 6, edges, D=2, P=2)
    # state s: dimension 0 uses parameter s % 2, dimension 1 parameter s // 2.  Sweep 0: state 0 = (1.0, 1.0) on [0, 4),
    # state 3 = (-2.0, -2.0) on [4, 6).  Sweep 1: band 0 everywhere in both dimensions.
    assert N == 2
    assert np.array_equal(counts, [[1, 1, 1, 1, 2, 2],      # d = 0, band 0
                                   [1, 1, 1, 1, 0, 0],      # d = 0, band 1
                                   [1, 1, 1, 1, 2, 2],      # d = 1, band 0
                                   [1, 1, 1, 1, 0, 0]])
    assert list(np.flatnonzero(boundary)) == [0, 4]          # (not 3: states 1 and 2 of sweep 1 share their bands)
    assert bu.level_segments(sweeps, 6) == 3
    length, seg = bu.rle(counts, boundary)
    assert list(length) == [4, 2] and np.array_equal(seg, [[1, 1, 1, 1], [2, 0, 2, 0]])
    assert np.array_equal(bu.cumulative(counts, 2, 2)[:, 0], [2, 1, 2, 1])
    assert np.array_equal(bu.exceedance(seg, 1, 2), [[1, 1], [0, 0]])
    # calls: rank 0 - the first maximum (a tie on the first segment: band 0); rank 1 - the smallest level's band; rank 2 = N
    for rank, want_len, want in ((0, [6], [[0], [0]]), (1, [6], [[0], [0]]), (2, [4, 2], [[1, 0], [1, 0]])):
        run_len, run_band = bu.call(seg, length, rank, 2, 2)
        assert list(run_len) == want_len and np.array_equal(run_band, want), rank
    assert bu.rank_of(0, 15) == 0 and bu.rank_of(0.5, 15) == 8 and bu.rank_of(1.0, 15) == 15 and bu.rank_of(0.001, 15) == 1
    assert bu.bands_text(length, seg) == "4\t1\t1\t1\t1\n2\t2\t0\t2\t0\n"
    assert bu.calls_text(*bu.call(seg, length, 2, 2, 2)) == "0 4 1 1\n4 2 0 0\n"


def test_exceedance_helper_of_the_package():
    from hammlet_amd import capi
    rng = np.random.RandomState(3)
    for D, n_edges in ((1, 2), (2, 1), (3, 9)):
        seg = rng.randint(0, 50, size=(17, D * (n_edges + 1))).astype(np.int32)
        got = capi.bands_exceedance(seg, n_edges, D)
        assert got.dtype == np.int64 and np.array_equal(got, bu.exceedance(seg, n_edges, D))


def test_helper_matches_the_checkers_marginals():
    """A chain whose means stay ordered and apart, with edges between them: band b IS the state with the b-th smallest mean, so
    the helper must reproduce OracleChain.marginals_dense() row by row after relabelling by mean; and in every case the
    columns of a dimension sum to N at every position."""
    T, K = 20000, 3
    x = ol.trace(T, K, 3)
    o = ol.OracleChain(K=K, seed=5, rng=ol.RNG_CTR, math=ol.MATH_DEV, reduce=ol.REDUCE_DEV)
    o.load(x)
    o.autoprior()
    o.init_model()
    o.set_record(marginals=True)
    o.token("F")
    o.iterate("F", 30, 0)                               # past the burn-in: the means have found the three levels
    sweeps = []
    for i in range(12):
        o.iterate("F", 1, 1)
        sweeps.append((o.blocks().copy(), o.states().copy(), o.theta()[0::2].copy()))
    edges = (-0.5, 0.5)
    order = np.argsort(sweeps[0][2])
    for _, _, mean in sweeps:
        assert np.array_equal(np.argsort(mean), order) and np.array_equal(bu.band_of(edges, mean[order]), [0, 1, 2])
    counts, boundary, N = bu.accumulate(sweeps, T, edges)
    dense = o.marginals_dense()
    assert N == 12 and np.array_equal(counts, dense[order].astype(np.int64))
    assert np.array_equal(counts.sum(axis=0), np.full(T, N))
    o.close()


@pytest.mark.parametrize("name", sorted(bc.CASES))
def test_gpu_cases_are_not_vacuous(name):
    """on the checker's chain alone: at least two bands populated in every dimension; a recorded sweep in which adjacent runs of
    different states share all bands, and strictly fewer band segments than level segments; a position whose band differs
    between two recorded sweeps; for the rank cases, calls at rank 1, ceil(N / 2) and N that are not all equal"""
    c = bc.CASES[name]
    T, D, edges = c["T"], c["D"], c["edges"]
    P = c["P"] if D > 1 else c["K"]
    nb = len(edges) + 1
    sweeps = bc.sweeps_of(name)
    counts, boundary, N = bu.accumulate(sweeps, T, edges, D=D, P=P)
    assert N == len(sweeps) > 1
    for d in range(D):
        rows = counts[d * nb:(d + 1) * nb]
        assert np.array_equal(rows.sum(axis=0), np.full(T, N))
        assert int(np.sum(rows.sum(axis=1) > 0)) >= 2, (name, d)
        assert np.any((rows > 0).sum(axis=0) >= 2), (name, d)      # a position whose band differs between two sweeps
    shared = 0
    for sweep in sweeps:
        pos, bands = bu.sweep_bands(sweep, edges, D, P)
        shared += int(np.sum(np.all(bands[:, 1:] == bands[:, :-1], axis=0)))
    assert shared > 0, name
    assert int(boundary.sum()) < bu.level_segments(sweeps, T), name
    if name in bc.RANK_CASES:
        length, seg = bu.rle(counts, boundary)
        calls = [bu.calls_text(*bu.call(seg, length, r, D, nb)) for r in (1, int(math.ceil(N / 2)), N)]
        assert len(set(calls)) > 1, name

"""Emission levels per position (include/hml.h: hml_set_level_recording, hml_levels_rle, hml_levels_dense_device,
hml_levels_merge) - what can be checked without a GPU: the library's surface, and the numpy accumulator of
tests/levels_util.py against the CPU checker's own marginals."""
import ctypes

import numpy as np
import pytest

from tests import levels_util as lu
from tests import oracle_lib as ol


def test_library_exports_the_level_calls():
    from hammlet_amd import build, capi
    build.build_library()
    lib = ctypes.CDLL(build.LIB_PATH)
    for name in ("hml_set_level_recording", "hml_levels_rle", "hml_levels_dense_device", "hml_levels_merge"):
        assert hasattr(lib, name), name
        assert name in capi.SIGNATURES
    lib.hml_abi_version.restype = ctypes.c_uint32
    assert lib.hml_abi_version() >= 4
    assert capi.ABI_VERSION == lib.hml_abi_version()
    for name in ("set_level_recording", "levels_rle", "levels_dense_device", "merge_levels"):
        assert hasattr(capi.Chain, name)


def test_levels_mean_sd_formula():
    from hammlet_amd import capi
    s1 = np.array([[3.0, -6.0, 0.0]])
    s2 = np.array([[5.0, 12.0, 0.0]])
    mean, sd = capi.levels_mean_sd(3, s1, s2)
    assert mean.dtype == np.float32 and sd.dtype == np.float32
    assert np.array_equal(mean, np.array([[1.0, -2.0, 0.0]], np.float32))
    assert np.array_equal(sd, np.sqrt(np.array([[5.0 / 3 - 1.0, 0.0, 0.0]])).astype(np.float32))
    # rounding may leave S2 / N a hair below the squared mean: the spread is zero then, not NaN
    mean, sd = capi.levels_mean_sd(3, np.array([[3.0]]), np.array([[3.0 * (1 - 2.0 ** -50)]]))
    assert sd[0, 0] == 0.0
    mean, sd = capi.levels_mean_sd(0, s1, s2)
    assert np.all(np.isnan(mean)) and np.all(np.isnan(sd))


def _chain(K, seed, x, mode, D=1, P=None, chain=0):
    rng, math, red = (ol.RNG_CTR, ol.MATH_DEV, ol.REDUCE_DEV) if mode == "device" else (ol.RNG_MT, ol.MATH_LIBM, ol.REDUCE_REF)
    o = ol.OracleChain(K=K, seed=seed, chain=chain, rng=rng, math=math, reduce=red)
    if D > 1:
        o.set_dimensions(D, P)
    o.load(x)
    o.autoprior()
    o.init_model()
    o.set_record(marginals=True)
    return o


def step_checker(o, scheme):
    """the scheme one sweep per call; returns (starts, states, means) of every recorded sweep"""
    sweeps = []
    for tok in scheme:
        if isinstance(tok, str):
            o.token(tok)
            continue
        m, n, t = tok
        for i in range(n):
            rec = t > 0 and (i + 1) % t == 0
            o.iterate(m, 1, 1 if rec else 0)
            if rec:
                sweeps.append((o.blocks().copy(), o.states().copy(), o.theta()[0::2].copy()))
    return sweeps


@pytest.mark.parametrize("T,K,D,P,mode,scheme", [
    (20000, 3, 1, None, "device", [("F", 12, 1)]),
    (20000, 4, 1, None, "device", [("M", 6, 2), "S", "P", ("F", 6, 0), ("F", 9, 3), "D", ("F", 4, 1)]),
    (12000, 4, 2, 2, "device", [("F", 10, 2)]),
    (15000, 3, 1, None, "reference", [("M", 5, 1), ("F", 8, 2)]),
])
def test_helper_matches_the_checkers_marginals(T, K, D, P, mode, scheme):
    """The helper's run boundaries and its per-sweep dense addition, fed the indicator of a state in place of mu, must
    reproduce OracleChain.marginals_dense() - after it is established that stepping the checker one sweep per call leaves the
    state that one call of n sweeps leaves."""
    if D > 1:
        x = np.stack([ol.trace(T, P, 50 + d) for d in range(D)], axis=1).reshape(-1)
    else:
        x = ol.trace(T, K, 3)
    whole = _chain(K, 5, x, mode, D, P)
    for tok in scheme:
        if isinstance(tok, str):
            whole.token(tok)
        else:
            whole.iterate(*tok)
    stepped = _chain(K, 5, x, mode, D, P)
    sweeps = step_checker(stepped, scheme)
    assert np.array_equal(whole.blocks(), stepped.blocks())
    assert np.array_equal(whole.states(), stepped.states())
    assert np.array_equal(whole.theta().view(np.uint32), stepped.theta().view(np.uint32))
    dense = stepped.marginals_dense()
    assert np.array_equal(dense, whole.marginals_dense())
    assert len(sweeps) == sum(tok[1] // tok[2] for tok in scheme if not isinstance(tok, str) and tok[2] > 0)
    for s in range(K):
        S1, S2, boundary, N = lu.accumulate(sweeps, T, D=1, value=lambda n, d, st, s=s: (st == s).astype(np.float64))
        assert np.array_equal(S1[0], dense[s].astype(np.float64)), s
        assert np.array_equal(S2[0], S1[0])
    # the union of run boundaries is where the checker's marginals file is cut
    pos, length = lu.segments(boundary)
    want = [int(line.split()[0]) for line in stepped.text("marginals").splitlines()]
    assert list(length) == want


def test_helper_levels_by_hand():
    """two sweeps on six positions, D = 2 over P = 2 parameters"""
    sweeps = [(np.array([0, 2, 4, 6]), np.array([0, 0, 3]), np.array([1.0, -2.0], np.float32)),
              (np.array([0, 3, 6]), np.array([1, 2]), np.array([0.5, 4.0], np.float32))]
    S1, S2, boundary, N = lu.accumulate(sweeps, 6, D=2, P=2)
    # state s: dimension 0 uses parameter s % 2, dimension 1 parameter s // 2
    assert np.array_equal(S1[0], [1 + 4, 1 + 4, 1 + 4, 1 + 0.5, -2 + 0.5, -2 + 0.5])
    assert np.array_equal(S1[1], [1 + 0.5, 1 + 0.5, 1 + 0.5, 1 + 4, -2 + 4, -2 + 4])
    assert np.array_equal(S2[0], [1 + 16, 1 + 16, 1 + 16, 1 + 0.25, 4 + 0.25, 4 + 0.25])
    assert N == 2 and list(np.flatnonzero(boundary)) == [0, 3, 4]
    assert np.array_equal(lu.param_of_state(4, 2, 2), [[0, 0], [1, 0], [0, 1], [1, 1]])


@pytest.mark.parametrize("M", [1, 3, 1023, 1024, 1025, 3038, (1 << 20) + 777])
def test_exact_scan_is_a_prefix_sum(M):
    """the restated tree on integers, where every order of additions gives the same sums, and on floats within rounding"""
    rng = np.random.default_rng(M)
    k = rng.integers(-9, 10, M).astype(np.float64)
    assert np.array_equal(lu.exact_scan(k), np.cumsum(k))
    x = rng.standard_normal(M)
    assert np.max(np.abs(lu.exact_scan(x) - np.cumsum(x))) <= 2.0 ** -52 * M * np.sum(np.abs(x))


@pytest.mark.parametrize("name", list(lu.EXACT_CASES))
def test_exact_cases_land_in_their_ranges(name):
    """the chains of test_levels_double_sums_exactly (tests/test_gpu_levels.py) on the checker: M lies in the regime of the
    scan's tree that the case is there for (asserted by exact_case_cells), and the restated read-outs agree with plain dense
    prefix sums within the levels' bounds"""
    kind, T, K, seed, chains, _ = lu.EXACT_CASES[name]
    x = lu.exact_case_trace(name)
    sweeps = [step_checker(_chain(K, seed, x, "device", chain=ch), scheme) for ch, scheme in chains]
    cells = lu.exact_case_cells(name, sweeps)
    pos, v = lu.exact_rle(cells)
    everything = [s for per_chain in sweeps for s in per_chain]
    S1, S2, boundary, N = lu.accumulate(everything, T)
    assert np.array_equal(np.flatnonzero(boundary), pos)
    E1, E2 = lu.bounds(pos.size, N, lu.max_abs_mean(everything))
    assert np.max(np.abs(v[0] - S1[0][pos])) <= E1 and np.max(np.abs(v[1] - S2[0][pos])) <= E2
    cuts = lu.exact_case_cuts(name, cells)
    assert cuts.size >= 8 and np.all(np.diff(cuts.astype(np.int64)) > 0)
    out = lu.exact_on_segments(cells, cuts)
    edges = np.concatenate(([0], cuts.astype(np.int64), [T]))
    for r, S in enumerate((S1[0], S2[0])):
        F = np.concatenate(([0.0], np.cumsum(S)))
        # (every term of a segment's sum carries a segment-sum error of at most E; T terms at most)
        assert np.max(np.abs(out[r] - (F[edges[1:]] - F[edges[:-1]]))) <= 4.0 * T * (E1, E2)[r] + 2.0 ** -50 * np.max(np.abs(F))

"""Agreement of chains on the emission level (include/hml.h: hml_levels_agreement_rle, hml_levels_agreement_dense_device,
hml_levels_agreement_summary) - what can be checked without a GPU: the library's surface, the formula of capi.levels_rhat on
values worked out by hand, and the run-length helper of tests/agreement_util.py against a position-by-position restatement."""
import ctypes

import numpy as np
import pytest

from tests import agreement_util as au
from tests import levels_util as lu
from tests import oracle_lib as ol
from tests.test_levels_cpu import _chain, step_checker

CALLS = ("hml_levels_agreement_rle", "hml_levels_agreement_dense_device", "hml_levels_agreement_summary")


def test_library_exports_the_agreement_calls():
    import hammlet_amd
    from hammlet_amd import build, capi
    build.build_library()
    lib = ctypes.CDLL(build.LIB_PATH)
    for name in CALLS:
        assert hasattr(lib, name), name
        assert name in capi.SIGNATURES
    lib.hml_abi_version.restype = ctypes.c_uint32
    assert lib.hml_abi_version() == 5 and capi.ABI_VERSION == 5    # additions only
    for name in ("levels_agreement_rle", "levels_agreement_dense_device", "levels_agreement_summary", "levels_rhat"):
        assert callable(getattr(capi, name)) and callable(getattr(hammlet_amd, name)), name


def _one(N, s1, s2):
    """levels_rhat for one segment of one dimension: s1, s2 per chain"""
    w, b, r = hml_rhat(N, np.asarray(s1, np.float64).reshape(-1, 1, 1), np.asarray(s2, np.float64).reshape(-1, 1, 1))
    assert w.shape == b.shape == r.shape == (1, 1) and w.dtype == b.dtype == r.dtype == np.float64
    return w[0, 0], b[0, 0], r[0, 0]


def hml_rhat(*args):
    from hammlet_amd import capi
    return capi.levels_rhat(*args)


def test_formula_by_hand():
    # two identical chains, N = 4 sweeps at levels 1, 1, 3, 3: S1 = 8, S2 = 20, m = 2, q = 5 - 4 = 1
    w, b, r = _one(4, [8.0, 8.0], [20.0, 20.0])
    assert b == 0.0 and w == 4.0 / 3.0 and r == np.sqrt(1.0 / (4.0 / 3.0))
    assert r < 1.0 and abs(r - np.sqrt(3.0 / 4.0)) <= 2.0 ** -52     # sqrt((N - 1) / N), up to the order of the operations
    # chains at 2 +- 1 and 4 +- 1: means 2 and 4, between = ((2 - 3)^2 + (4 - 3)^2) / 1 = 2, w0 = 1
    w, b, r = _one(4, [8.0, 16.0], [20.0, 68.0])
    assert b == 2.0 and w == 4.0 / 3.0 and r == np.sqrt(3.0 / (4.0 / 3.0))
    # three chains: means 0, 3, 6 without spread - within == 0 and between == 9 > 0: +inf
    w, b, r = _one(2, [0.0, 6.0, 12.0], [0.0, 18.0, 72.0])
    assert w == 0.0 and b == 9.0 and np.isposinf(r)
    # nothing moves anywhere: within == 0 and between == 0: 1
    w, b, r = _one(5, [10.0, 10.0], [20.0, 20.0])
    assert w == 0.0 and b == 0.0 and r == 1.0
    # rounding may leave S2 / N a hair below the squared mean: q = 0, not negative, and no NaN
    w, b, r = _one(3, [3.0, 3.0], [3.0 * (1 - 2.0 ** -50), 3.0])
    assert w == 0.0 and b == 0.0 and r == 1.0
    w, b, r = _one(3, [3.0, 6.0], [3.0 * (1 - 2.0 ** -50), 12.0])
    assert w == 0.0 and b == 0.5 and np.isposinf(r)
    # shapes [n][D][U] in, [D][U] out; every entry on its own
    s1 = np.array([[[8.0, 10.0], [0.0, 3.0]], [[16.0, 10.0], [6.0, 6.0]]])
    s2 = np.array([[[20.0, 20.0], [0.0, 3.0]], [[68.0, 20.0], [18.0, 12.0]]])
    w, b, r = hml_rhat(4, s1, s2)
    assert w.shape == (2, 2)
    for d in range(2):
        for u in range(2):
            assert (w[d, u], b[d, u], r[d, u]) == _one(4, s1[:, d, u], s2[:, d, u])


def test_hand_made_sweeps():
    """chain A sits at level 0 and chain B at level 1 on the first half, both jitter around 0 on the second half: R-hat is
    above 5 on the first half and below 1.2 on the second, and the union is cut where either chain is"""
    T, N = 400, 40
    rng = np.random.default_rng(3)

    def sweeps(base, cuts):
        out = []
        for _ in range(N):
            jit = (0.05 * rng.standard_normal(3)).astype(np.float32)
            mean = np.array([base + jit[0], jit[1], jit[2]], np.float32)   # state 0: the first half
            out.append((np.array([0] + cuts + [T]), np.arange(len(cuts) + 1) % 3, mean))
        return out

    A = lu.accumulate(sweeps(0.0, [T // 2]), T)                   # cut at T / 2
    B = lu.accumulate(sweeps(1.0, [T // 2, 3 * T // 4]), T)       # ... and at 3 T / 4: states 0, 1, 2
    rle = []
    for S1, S2, boundary, n in (A, B):
        seg, s1, s2 = au.rle_of_dense(S1, S2, boundary)
        rle.append((seg, n, s1, s2))
    seg, within, between, rhat = au.agreement_from_rle(rle, T)
    assert list(seg) == [T // 2, T // 4, T // 4]
    assert rhat[0, 0] > 5.0 and np.all(rhat[0, 1:] < 1.2) and np.all(rhat[0, 1:] > 0.9)
    assert abs(between[0, 0] - 0.5) < 0.02 and np.all(within[0] > 0)
    # the same through the position-by-position form
    _, _, dense = au.agreement_dense(N, np.stack([A[0], B[0]]), np.stack([A[1], B[1]]))
    assert np.array_equal(au.bits64(np.repeat(rhat, seg, axis=1)), au.bits64(dense))


@pytest.mark.parametrize("n_chains,D", [(2, 1), (3, 1), (2, 2), (3, 2)])
def test_rle_helper_equals_dense_brute_force(n_chains, D):
    """checker chains with different chain ids, three emission parameters (D = 2: `-s C 3 2`, nine states): the helper on the
    chains' run-length levels, expanded by the union's lengths, equals the position-by-position form bit for bit"""
    T, P, seed = 20000, 3, 5
    K = P ** D
    scheme = [("F", 12, 1)]
    if D > 1:
        x = np.stack([ol.trace(T, P, 50 + d) for d in range(D)], axis=1).reshape(-1)
    else:
        x = ol.trace(T, P, 3)
    acc = [lu.accumulate(step_checker(_chain(K, seed, x, "device", D, P if D > 1 else None, chain=ch), scheme), T, D=D, P=P)
           for ch in range(n_chains)]
    N = acc[0][3]
    assert N == 12
    rle = []
    for S1, S2, boundary, n in acc:
        seg, s1, s2 = au.rle_of_dense(S1, S2, boundary)
        rle.append((seg, n, s1, s2))
    seg, within, between, rhat = au.agreement_from_rle(rle, T)
    union = np.zeros(T, bool)
    for a in acc:
        union |= a[2]
    assert np.array_equal(au.starts_of(seg), np.flatnonzero(union)) and seg.sum() == T
    assert any(len(r[0]) < len(seg) for r in rle)          # the chains cut in different places
    dw, db, dr = au.agreement_dense(N, np.stack([a[0] for a in acc]), np.stack([a[1] for a in acc]))
    for got, want in ((within, dw), (between, db), (rhat, dr)):
        assert got.shape == (D, len(seg))
        assert np.array_equal(au.bits64(np.repeat(got, seg, axis=1)), au.bits64(want))
    assert np.all(rhat > 0) and np.any(np.isfinite(rhat))

"""Agreement of chains on the emission level on the GPU (hml_k_agree.h behind hml_levels_agreement_rle /
hml_levels_agreement_dense_device / hml_levels_agreement_summary).  The expected values come from tests/agreement_util.py fed
the chains' OWN levels_rle() outputs - the union of their starts, their values repeated onto it, capi.levels_rhat: within and
between bit for bit, rhat within 2 units in the last place (the device's double square root is not pinned as correctly rounded)."""
import ctypes

import numpy as np
import pytest

from tests import agreement_util as au
from tests import hostile_inputs as hi
from tests import levels_util as lu
from tests import oracle_lib as ol

pytestmark = pytest.mark.gpu


def gpu_chain(hml, K, seed, x, chain=0, D=1, P=None, levels=True, attach=None):
    g = hml.Chain(device=0, seed=seed, chain_id=chain)
    if attach is not None:
        g.attach(attach)
    else:
        if D > 1:
            g.set_dimensions(D, P)
        g.load(x)
    g.set_model(K, g.autoprior(0.2, 0.9))
    if levels:
        g.set_level_recording(True)
    g.sample_prior()
    return g


def run_scheme(g, scheme):
    for tok in scheme:
        g.iterate(*tok)
    g.sync()
    return g


def private_chains(hml, x, K, seed, scheme, ids, D=1, P=None):
    return [run_scheme(gpu_chain(hml, K, seed, x, chain=ch, D=D, P=P), scheme) for ch in ids]


def attached_chains(hml, x, K, seed, scheme, ids):
    first = gpu_chain(hml, K, seed, x, chain=ids[0])
    chains = [first] + [gpu_chain(hml, K, seed, x, chain=ch, attach=first) for ch in ids[1:]]
    for m, n, t in scheme:
        hml.iterate_many(chains, m, n, t)
    for g in chains:
        g.sync()
    return chains


def assert_agreement(hml, chains, what=""):
    """the device's agreement of `chains` against the helper fed their levels_rle(); returns what the device returned"""
    T = chains[0].T
    rle = [g.levels_rle() for g in chains]
    seg, n, within, between, rhat = hml.levels_agreement_rle(chains)
    want_seg, want_w, want_b, want_r = au.agreement_from_rle(rle, T)
    assert n == rle[0][1], (what, n)
    assert np.array_equal(seg.astype(np.int64), want_seg), what
    assert within.shape == between.shape == rhat.shape == (chains[0].D, len(seg))
    diff_w = int(np.sum(au.bits64(within) != au.bits64(want_w)))
    diff_b = int(np.sum(au.bits64(between) != au.bits64(want_b)))
    inf = np.isinf(want_r)
    ulps = int(np.max(au.ulps64(rhat[~inf], want_r[~inf]))) if np.any(~inf) else 0
    print("%s: U=%d (chains: %s), N=%d; entries with other bits: within %d, between %d; rhat at most %d ulp off, %d infinite, largest finite %.4g"
          % (what, len(seg), " ".join(str(len(r[0])) for r in rle), n, diff_w, diff_b, ulps, int(inf.sum()), float(np.max(rhat[~inf])) if np.any(~inf) else 0.0))
    assert diff_w == 0 and diff_b == 0, (what, diff_w, diff_b)
    assert np.array_equal(np.isinf(rhat), inf) and np.all(rhat[inf] > 0), what
    assert not np.any(np.isnan(rhat)) and ulps <= 2, (what, ulps)
    return seg, n, within, between, rhat


@pytest.fixture(scope="module")
def trio(hml):
    """three chains attached to one trace and driven by hml_iterate_many; read only by the tests that share it"""
    T, K = 80000, 5
    return attached_chains(hml, ol.trace(T, K, 7), K, 21, [("F", 12, 1)], [0, 1, 2])


@pytest.fixture(scope="module")
def pair_2d(hml):
    """`-s C 2 2`: two private chains over two data dimensions"""
    T, P, D = 40000, 2, 2
    x = np.stack([ol.trace(T, P, 9 + d) for d in range(D)], axis=1).reshape(-1)
    return private_chains(hml, x, P ** D, 6, [("F", 12, 1)], [0, 1], D=D, P=P)


def test_agreement_two_private_chains(hml):
    T, K = 20000, 3
    chains = private_chains(hml, ol.trace(T, K, 7), K, 42, [("F", 12, 1)], [0, 1])
    seg, n, within, between, rhat = assert_agreement(hml, chains, "n=2 private")
    assert n == 12 and len(seg) >= max(len(g.levels_rle()[0]) for g in chains) > 1


def test_agreement_three_attached_chains(hml, trio):
    seg, n, within, between, rhat = assert_agreement(hml, trio, "n=3 attached, iterate_many")
    assert n == 12 and len(seg) > 1


def test_agreement_two_dimensions(hml, pair_2d):
    seg, n, within, between, rhat = assert_agreement(hml, pair_2d, "D=2 P=2")
    assert rhat.shape[0] == 2 and not np.array_equal(rhat[0], rhat[1])


# The rank scan's tree (hml_k_scan.h) over the union's U entries: one partial chunk, several chunks, more than 2^20 entries
# (chunk totals in pieces of two), and the two-position trace.  (trace, T, K, seed, scheme, least U, most U)
REGIMES = {
    "one_partial_chunk": ("depth", 200, 5, 17, [("M", 4, 0), ("F", 6, 2)], 2, 255),
    "several_chunks": ("depth", 4000, 5, 17, [("M", 4, 0), ("F", 6, 2)], 1025, 4095),
    "pieces_of_two_chunks": ("depth", 4000000, 5, 17, [("M", 1, 1), ("F", 2, 1)], (1 << 20) + 1, 1 << 22),
    "tiny_2": ("tiny_2", 2, 2, 12, [("F", 10, 1)], 1, 2),
}
assert REGIMES["pieces_of_two_chunks"][:4] == lu.EXACT_CASES["pieces_of_two_chunks"][:4]
assert REGIMES["pieces_of_two_chunks"][4] == lu.EXACT_CASES["pieces_of_two_chunks"][4][0][1]


@pytest.mark.parametrize("name", list(REGIMES))
def test_agreement_in_every_regime_of_the_rank_scan(hml, name):
    kind, T, K, seed, scheme, lo, hi_ = REGIMES[name]
    x = hi.data(name) if kind == "tiny_2" else ol.synth_depth(T, seed=5)
    chains = private_chains(hml, x, K, seed, scheme, [0, 1])
    seg, n, within, between, rhat = assert_agreement(hml, chains, name)
    assert lo <= len(seg) <= hi_, (name, len(seg))
    assert seg.sum() == T
    # the summary and the dense form on the same union
    above, largest, infinite = hml.levels_agreement_summary(chains, 1.1)
    assert above[0] == int(seg[rhat[0] > 1.1].sum()) and infinite[0] == int(seg[np.isinf(rhat[0])].sum())


def test_agreement_leaves_the_contexts_unchanged(hml):
    import torch
    T, K = 30000, 4
    chains = private_chains(hml, ol.trace(T, K, 7), K, 13, [("F", 8, 1)], [0, 1, 2])
    before = [g.levels_rle() for g in chains]
    first = hml.levels_agreement_rle(chains)
    out = torch.empty((1, T), dtype=torch.float32, device="cuda:0")
    hml.levels_agreement_dense_device(chains, out.data_ptr())
    hml.levels_agreement_summary(chains, 1.1)
    again = hml.levels_agreement_rle(chains)
    for a, b in zip(first, again):
        assert np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))
    for g, (seg, n, s1, s2) in zip(chains, before):
        seg2, n2, t1, t2 = g.levels_rle()
        assert n2 == n == 8 and np.array_equal(seg, seg2)
        assert np.array_equal(au.bits64(s1), au.bits64(t1)) and np.array_equal(au.bits64(s2), au.bits64(t2))
    # the chains record on
    for g in chains:
        g.iterate("F", 2, 1)
        g.sync()
        assert g.levels_rle()[1] == 10
    assert_agreement(hml, chains, "after two more sweeps")
    # one chain a sweep ahead: refused
    chains[1].iterate("F", 1, 1)
    chains[1].sync()
    for call in (lambda: hml.levels_agreement_rle(chains), lambda: hml.levels_agreement_summary(chains, 1.1),
                 lambda: hml.levels_agreement_dense_device(chains, out.data_ptr())):
        with pytest.raises(hml.HmlError) as e:
            call()
        assert e.value.code == 1 and "same number of recorded sweeps" in str(e.value)


def test_agreement_refusals(hml):
    import torch
    T, K = 20000, 3
    x = ol.trace(T, K, 7)
    a, b = private_chains(hml, x, K, 5, [("F", 4, 1)], [0, 1])
    messages = []

    def refused(chains, call=None):
        with pytest.raises(hml.HmlError) as e:
            (call or hml.levels_agreement_rle)(chains)
        assert e.value.code == 1, str(e.value)
        messages.append(str(e.value))

    # a null argument: the array, an element, an output
    lib = hml.load_library()
    u, n = ctypes.c_uint64(), ctypes.c_uint64()
    assert lib.hml_levels_agreement_rle(None, 2, ctypes.byref(u), ctypes.byref(n), None, None, None, None) == 1
    assert "null argument" in lib.hml_last_error().decode()
    arr = (ctypes.c_void_p * 2)(a.h, None)
    assert lib.hml_levels_agreement_rle(ctypes.cast(arr, ctypes.c_void_p), 2, ctypes.byref(u), ctypes.byref(n), None, None, None, None) == 1
    arr = (ctypes.c_void_p * 2)(a.h, b.h)
    assert lib.hml_levels_agreement_rle(ctypes.cast(arr, ctypes.c_void_p), 2, None, ctypes.byref(n), None, None, None, None) == 1
    assert lib.hml_levels_agreement_summary(ctypes.cast(arr, ctypes.c_void_p), 2, 1.1, None, None, None) == 1
    refused([a, b], lambda ch: hml.levels_agreement_dense_device(ch, None))
    # n outside 2 .. 64
    refused([a])
    refused([a, b] * 33)
    assert messages[-1] == messages[-2]
    messages.pop()
    # a context given twice
    refused([a, b, a])
    # other positions, other dimensions
    short = private_chains(hml, x[:10000], K, 5, [("F", 4, 1)], [1])[0]
    refused([a, short])
    two_d = private_chains(hml, np.stack([ol.trace(T, 2, 9), ol.trace(T, 2, 10)], axis=1).reshape(-1), 4, 5, [("F", 4, 1)], [1], D=2, P=2)[0]
    refused([a, two_d])
    assert messages[-1] == messages[-2]
    messages.pop()
    # a context that never recorded levels
    never = run_scheme(gpu_chain(hml, K, 5, x, chain=2, levels=False), [("F", 4, 1)])
    refused([a, never])
    assert "hml_set_level_recording" in messages[-1]
    # fewer than two recorded sweeps: one, and none
    one = private_chains(hml, x, K, 5, [("F", 1, 1)], [2, 3])
    refused(one)
    none = private_chains(hml, x, K, 5, [("F", 2, 0)], [2, 3])
    refused(none)
    assert messages[-1] == messages[-2] and "at least two recorded sweeps" in messages[-1]
    messages.pop()
    # unequal numbers of recorded sweeps
    longer = private_chains(hml, x, K, 5, [("F", 6, 1)], [2])[0]
    refused([a, longer])
    # chains on different GPUs, where there are two
    if torch.cuda.device_count() >= 2:
        far = hml.Chain(device=1, seed=5, chain_id=1)
        far.load(x)
        far.set_model(K, far.autoprior(0.2, 0.9))
        far.set_level_recording(True)
        far.sample_prior()
        run_scheme(far, [("F", 4, 1)])
        refused([a, far])
        assert "different GPUs" in messages[-1]
    assert len(set(messages)) == len(messages), messages       # a message of its own for each
    # ... and the chains still answer
    assert_agreement(hml, [a, b], "after the refusals")


def test_agreement_of_a_chain_with_its_copy(hml):
    """the same seed and chain id in two contexts: between == 0 exactly, every rhat = sqrt(w0 / within) < 1"""
    T, K = 30000, 4
    x = ol.trace(T, K, 7)
    chains = private_chains(hml, x, K, 13, [("F", 10, 1)], [3, 3])
    seg, n, within, between, rhat = assert_agreement(hml, chains, "a chain and its copy")
    assert np.all(between == 0.0) and np.all(rhat < 1.0)
    above, largest, infinite = hml.levels_agreement_summary(chains, 1.0)
    assert above[0] == 0 and infinite[0] == 0 and largest[0] == np.max(rhat)


def test_agreement_is_label_invariant(hml, oracle):
    """The permuted-label construction of test_levels_are_label_invariant (tests/test_gpu_levels.py): chain B with its states
    renamed - parameters, rows and columns of A and pi permuted alike - static blocks, probes, recorded sweeps.  A renamed run is
    not the same draw (the backward pass inverts the cumulative sums over the states in label order, and the parameter draws are
    keyed by label), so `the same bits for (A, B) and (A, renamed B)` cannot be asked of two runs.  What is asked, under either
    naming: B's levels are the CPU checker's label-free levels of the same run within the levels' bounds (levels_util.accumulate
    sees mu(q_t) alone, never a label), and the agreement of (A, B) is bit for bit the helper's answer from those levels - a
    function of the levels and of nothing else."""
    from tests.test_gpu_levels import checker
    T, K, seed = 60000, 4, 9
    x = ol.trace(T, K, 7)
    perm = np.array([2, 0, 3, 1])
    A = private_chains(hml, x, K, seed, [("F", 10, 0), ("F", 3, 1)], [1])[0]
    for renamed in (False, True):
        o = checker(K, seed, x)
        g = gpu_chain(hml, K, seed, x)
        o.token("F")
        o.iterate("F", 10, 0)
        g.iterate("F", 10, 0)
        mv, (Am, pi) = g.theta().reshape(K, 2), g.transitions()
        if renamed:
            mv, Am, pi = mv[perm], Am[np.ix_(perm, perm)], pi[perm]
        o.set_params(mv.reshape(-1), Am, pi)
        g.set_parameters(mv.reshape(-1), Am, pi)
        o.token("S")
        g.set_static_blocks()
        o.set_probes(True)
        g.enable_probes(True)
        sweeps = []
        for _ in range(3):
            o.iterate("F", 1, 0)
            g.iterate("F", 1, 1)
            g.sync()
            assert np.array_equal(o.states(), g.states())
            sweeps.append((o.blocks().copy(), o.states().copy(), o.theta()[0::2].copy()))
        seg, n, s1, s2 = g.levels_rle()
        S1, S2, boundary, N = lu.accumulate(sweeps, T)
        pos, length = lu.segments(boundary)
        E1, E2 = lu.bounds(len(seg), N, lu.max_abs_mean(sweeps))
        assert n == N == 3 and np.array_equal(seg.astype(np.int64), length), renamed
        assert np.max(np.abs(s1[0] - S1[0][pos])) <= E1 and np.max(np.abs(s2[0] - S2[0][pos])) <= E2, renamed
        assert_agreement(hml, [A, g], "renamed" if renamed else "original")


def test_agreement_dense_device(hml, pair_2d):
    """into a torch buffer pre-filled with -7: float32(rhat) repeated by the lengths, within one float unit in the last place
    (rhat itself is within 2 double units of numpy's); +inf stays +inf"""
    import torch
    chains = pair_2d
    T, D = chains[0].T, 2
    seg, n, within, between, rhat = hml.levels_agreement_rle(chains)
    out = torch.full((D, T), -7.0, dtype=torch.float32, device="cuda:0")
    hml.levels_agreement_dense_device(chains, out.data_ptr())
    got = out.cpu().numpy()
    want = np.repeat(rhat.astype(np.float32), seg.astype(np.int64), axis=1)
    assert got.shape == want.shape and not np.any(got == -7.0)
    inf = np.isinf(want)
    assert np.array_equal(np.isinf(got), inf) and np.all(got[inf] > 0)
    ulp = np.abs(got[~inf].view(np.int32).astype(np.int64) - want[~inf].view(np.int32).astype(np.int64))
    assert ulp.max() <= 1, int(ulp.max())
    # ... and the helper's value from the chains' own levels, the same way
    _, _, _, want_r = au.agreement_from_rle([g.levels_rle() for g in chains], T)
    want = np.repeat(want_r.astype(np.float32), seg.astype(np.int64), axis=1)
    ulp = np.abs(got[~inf].view(np.int32).astype(np.int64) - want[~inf].view(np.int32).astype(np.int64))
    assert np.array_equal(np.isinf(want), inf) and ulp.max() <= 1, int(ulp.max())


@pytest.mark.parametrize("which", ["trio", "pair_2d"])
def test_agreement_summary(hml, trio, pair_2d, which):
    """n_above, n_infinite and max_finite are what numpy derives from the rhat and seg_len of the run-length call, exactly:
    the same kernel, the same bits"""
    chains = trio if which == "trio" else pair_2d
    seg, n, within, between, rhat = hml.levels_agreement_rle(chains)
    seg = seg.astype(np.int64)
    finite = np.where(np.isfinite(rhat), rhat, 0.0)
    top = float(finite.max())
    for threshold in (1.0, 1.1, 2.0 * top):
        above, largest, infinite = hml.levels_agreement_summary(chains, threshold)
        for d in range(chains[0].D):
            assert above[d] == int(seg[rhat[d] > threshold].sum()), (threshold, d)
            assert infinite[d] == int(seg[np.isinf(rhat[d])].sum()), (threshold, d)
            assert largest[d] == finite[d].max(), (threshold, d)
        if threshold > top:
            assert np.array_equal(above, infinite)
    above, largest, infinite = hml.levels_agreement_summary(chains, 1.0)
    assert np.all(above <= chains[0].T)

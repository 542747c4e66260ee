"""Emission levels per position on the GPU (hml_k_levels.h behind hml_set_level_recording / hml_levels_rle /
hml_levels_dense_device / hml_levels_merge).  The expected sums come from the CPU CHECKER - its blocks, states and theta
after every recorded sweep, stepped one sweep per call (tests/test_levels_cpu.py shows that this is the same chain) -
accumulated by tests/levels_util.py; never from the product.

Bound of every segment sum: E1 = 2^-52 M N (N + 1) max|mu| for the level, E2 likewise with max mu^2 (M segments, N recorded
sweeps, the maximum over all recorded theta): at most N rounded additions of terms of at most 2 max into a cell, then at
most M rounded additions in the scan.  From the arithmetic, not from a measurement."""
import numpy as np
import pytest

from tests import hostile_inputs as hi
from tests import levels_util as lu
from tests import oracle_lib as ol

pytestmark = pytest.mark.gpu


def bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def checker(K, seed, x, chain=0, D=1, P=None, compat=False):
    mode = (ol.RNG_MT, ol.MATH_LIBM, ol.REDUCE_REF) if compat else (ol.RNG_CTR, ol.MATH_DEV, ol.REDUCE_DEV)
    o = ol.OracleChain(K=K, seed=seed, chain=chain, rng=mode[0], math=mode[1], reduce=mode[2])
    if D > 1:
        o.set_dimensions(D, P)
    o.load(x)
    o.autoprior()
    o.init_model()
    return o


def gpu_chain(hml, K, seed, x, chain=0, D=1, P=None, compat=False, options=(), levels=True, attach=None):
    g = hml.Chain(device=0, seed=seed, chain_id=chain)
    for name, value in options:
        g.set_option(name, value)
    if compat:
        g.set_option("compat", 1)
    if attach is not None:
        g.attach(attach)
    else:
        if D > 1:
            g.set_dimensions(D, P)
        g.load(x)
    g.set_model(K, g.autoprior(0.2, 0.9))
    if levels:
        g.set_level_recording(True)
    g._pending_prior = True
    return g


def gpu_token(g, tok):
    """one scheme token on the GPU chain: ONE iterate call per sweep token"""
    if g._pending_prior:
        g.sample_prior()
        g._pending_prior = False
    if tok == "P":
        g._pending_prior = True
    elif tok == "S":
        g.set_static_blocks()
    elif tok == "D":
        g.set_dynamic(True)
    else:
        g.iterate(*tok)


def checker_sweeps(o, scheme, after_token=None):
    """the checker through the scheme one sweep per call: (starts, states, means) of every recorded sweep"""
    sweeps = []
    for tok in scheme:
        if isinstance(tok, str):
            o.token(tok)
        else:
            m, n, t = tok
            for i in range(n):
                o.iterate(m, 1, 0)
                if t > 0 and (i + 1) % t == 0:
                    sweeps.append((o.blocks().copy(), o.states().copy(), o.theta()[0::2].copy()))
    return sweeps


def expected(sweeps, T, D, P):
    S1, S2, boundary, N = lu.accumulate(sweeps, T, D=D, P=P)
    pos, length = lu.segments(boundary)
    return S1, S2, pos, length, N


def assert_levels(g, sweeps, T, D=1, P=None, what=""):
    """levels_rle() of the GPU chain against the helper fed the checker's sweeps; returns what levels_rle() returned"""
    seg, n, s1, s2 = g.levels_rle()
    S1, S2, pos, length, N = expected(sweeps, T, D, P)
    assert n == N, (what, n, N)
    assert np.array_equal(seg.astype(np.int64), length), what
    M = len(seg)
    E1, E2 = lu.bounds(M, N, lu.max_abs_mean(sweeps))
    for d in range(D):
        err1 = float(np.max(np.abs(s1[d] - S1[d][pos])))
        err2 = float(np.max(np.abs(s2[d] - S2[d][pos])))
        print("%s d=%d M=%d N=%d: |S1 error| %.3g (bound %.3g), |S2 error| %.3g (bound %.3g)" % (what, d, M, N, err1, E1, err2, E2))
        assert err1 <= E1, (what, d, err1, E1)
        assert err2 <= E2, (what, d, err2, E2)
    return seg, n, s1, s2


def run_case(hml, x, K, seed, scheme, T, D=1, P=None, compat=False, options=(), chain=0, what=""):
    o = checker(K, seed, x, chain=chain, D=D, P=P, compat=compat)
    g = gpu_chain(hml, K, seed, x, chain=chain, D=D, P=P, compat=compat, options=options)
    sweeps = checker_sweeps(o, scheme)
    for tok in scheme:
        gpu_token(g, tok)
    g.sync()
    assert np.array_equal(o.blocks(), g.blocks()) and np.array_equal(o.states(), g.states()), what
    assert np.array_equal(o.theta().view(np.uint32), g.theta().view(np.uint32)), what
    out = assert_levels(g, sweeps, T, D=D, P=(P if D > 1 else K), what=what)
    return g, sweeps, out


MIXED = [("M", 6, 2), "S", "P", ("F", 6, 0), ("F", 9, 3), "D", ("F", 4, 1)]


@pytest.mark.parametrize("T,K,scheme", [
    (100000, 3, [("F", 30, 1)]),
    (200000, 5, [("F", 25, 5)]),
    (50000, 10, [("F", 10, 2)]),
    (30000, 16, [("F", 6, 2)]),
    (60000, 20, [("F", 12, 3)]),          # more than 16 states: sweep_wide
    (30000, 40, [("M", 4, 1), "S", "P", ("F", 8, 2), "D", ("F", 3, 1)]),
    (20000, 4, MIXED),
    (30000, 20, MIXED),
])
def test_levels_match_checker(hml, T, K, scheme):
    x = ol.trace(T, K if K in ol.LEVELS else 6, 7)
    run_case(hml, x, K, 42, scheme, T, what="K=%d" % K)


def test_levels_on_depth_data(hml):
    """the read-depth trace of test_sweeps_match_checker_on_depth_data: 1.4 positions per block"""
    T, K = 300000, 5
    x = ol.synth_depth(T, seed=5)
    run_case(hml, x, K, 17, [("M", 10, 0), ("F", 30, 3)], T, what="depth")


def test_levels_two_dimensions(hml):
    """`-s C 2 2`: four states over two parameters and two data dimensions"""
    T, P, D = 40000, 2, 2
    x = np.stack([ol.trace(T, P, 9 + d) for d in range(D)], axis=1).reshape(-1)
    g, sweeps, (seg, n, s1, s2) = run_case(hml, x, P ** D, 6, [("M", 5, 1), ("F", 15, 2)], T, D=D, P=P, what="C 2 2")
    assert s1.shape == (2, len(seg)) and not np.array_equal(s1[0], s1[1])


@pytest.mark.parametrize("thinning", [1, 3, 50])
def test_levels_thinning(hml, thinning):
    """thinning 1, 3, and beyond the number of sweeps: nothing recorded - one segment, zero sums, N = 0"""
    T, K = 50000, 3
    x = ol.trace(T, K, 7)
    g, sweeps, (seg, n, s1, s2) = run_case(hml, x, K, 11, [("F", 20, thinning)], T, what="thinning %d" % thinning)
    assert n == 20 // thinning
    if thinning == 50:
        assert n == 0 and list(seg) == [T] and s1[0, 0] == 0.0 and s2[0, 0] == 0.0


@pytest.mark.parametrize("case", ["k4_mixed_scheme", "mv_c22"])
def test_levels_reference_compatible_mode(hml, case):
    """compat = 1 (the update precedes the record there) against the checker in REFERENCE mode, on two golden configurations
    (tests/golden/manifest.json): `-s 4 -R 3 -i M 50 5 D F 60 2 P M 10 1 S F 30 1` and `-s C 2 2 -R 5 -i F 50 1`"""
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "manifest.json")) as f:
        m = json.load(f)[case]
    T, D = m["T"], m["dims"]
    if D == 1:
        assert m["flags"] == "-s 4 -R 3 -i M 50 5 D F 60 2 P M 10 1 S F 30 1"
        x, K, P, seed = ol.trace(T, m["trace_levels"], m["data_seed"]), 4, None, 3
        scheme = [("M", 50, 5), "D", ("F", 60, 2), "P", ("M", 10, 1), "S", ("F", 30, 1)]
    else:
        assert m["flags"] == "-s C 2 2 -R 5 -i F 50 1"
        x = np.stack([ol.trace(T, m["trace_levels"], m["data_seed"] + d) for d in range(D)], axis=1).reshape(-1)
        K, P, seed, scheme = 4, 2, 5, [("F", 50, 1)]
    run_case(hml, x, K, seed, scheme, T, D=D, P=P, compat=True, what="compat " + case)


def test_levels_iterate_many_equals_iterate_bit_for_bit(hml):
    """three chains attached to one trace through hml_iterate_many (the level kernel runs per chain behind the batch's
    parameter kernels): each chain's levels are those of the same chain alone under hml_iterate, bit for bit - and the checker's"""
    T, K, seed = 200000, 5, 21
    x = ol.trace(T, K, 7)
    scheme = [("F", 12, 0), ("F", 18, 3)]
    alone = []
    for k in range(3):
        g = gpu_chain(hml, K, seed, x, chain=k)
        for tok in scheme:
            gpu_token(g, tok)
        g.sync()
        alone.append(g.levels_rle())
        g.close()
    first = gpu_chain(hml, K, seed, x, chain=0)
    chains = [first] + [gpu_chain(hml, K, seed, x, chain=k, attach=first) for k in (1, 2)]
    for g in chains:
        g.sample_prior()
        g._pending_prior = False
    for m, n, t in scheme:
        hml.iterate_many(chains, m, n, t)
    for k, g in enumerate(chains):
        g.sync()
        seg, n, s1, s2 = g.levels_rle()
        assert n == alone[k][1] == 6
        assert np.array_equal(seg, alone[k][0]), k
        assert np.array_equal(bits64(s1), bits64(alone[k][2])) and np.array_equal(bits64(s2), bits64(alone[k][3])), k
    o = checker(K, seed, x, chain=1)
    assert_levels(chains[1], checker_sweeps(o, scheme), T, what="iterate_many chain 1")


def _levels_of(hml, x, K, seed, scheme, options=(), chain=0):
    g = gpu_chain(hml, K, seed, x, chain=chain, options=options)
    for tok in scheme:
        gpu_token(g, tok)
    g.sync()
    return g, g.levels_rle()


def test_levels_reproducible(hml):
    """two identical runs: the same bits; also with the fused block kernel off, and - on weakly compressed input, where the
    fused trellis kernels run - with two forced chunk lengths"""
    T, K = 150000, 5
    x = ol.trace(T, K, 7)
    scheme = [("F", 20, 2)]
    ref = _levels_of(hml, x, K, 3, scheme)[1]
    for options in ((), (("fused_blocks", 0),), (("fused_blocks", 1),)):
        got = _levels_of(hml, x, K, 3, scheme, options)[1]
        assert got[1] == ref[1] and np.array_equal(got[0], ref[0]), options
        assert np.array_equal(bits64(got[2]), bits64(ref[2])) and np.array_equal(bits64(got[3]), bits64(ref[3])), options
    T = 8_000_000                          # 1.4 positions per block: beyond dense_min_blocks = 2^22
    x = ol.synth_depth(T, seed=5)
    runs = []
    for L in (64, 256):
        g, lev = _levels_of(hml, x, K, 4, [("F", 4, 2)], (("trellis_L", L),))
        assert g.num_blocks() >= 1 << 22
        runs.append(lev)
    assert runs[0][1] == runs[1][1] == 2 and np.array_equal(runs[0][0], runs[1][0])
    assert np.array_equal(bits64(runs[0][2]), bits64(runs[1][2])) and np.array_equal(bits64(runs[0][3]), bits64(runs[1][3]))


def test_levels_survive_buffer_growth(hml):
    """a block capacity far below what the sweeps need: the chain halts, grows and runs the sweeps again (hml_settle) - every
    recorded sweep must be counted once: bit-identical to the run with the default capacity"""
    T, K = 100000, 3
    x = ol.trace(T, K, 7)
    scheme = [("M", 4, 1), ("F", 16, 2)]
    g0, ref = _levels_of(hml, x, K, 8, scheme)
    assert g0.stats()["buffer_growths"] == 0
    g1, got = _levels_of(hml, x, K, 8, scheme, (("max_blocks", 64),))
    assert g1.stats()["buffer_growths"] > 0
    assert got[1] == ref[1] == 12 and np.array_equal(got[0], ref[0])
    assert np.array_equal(bits64(got[2]), bits64(ref[2])) and np.array_equal(bits64(got[3]), bits64(ref[3]))


def dense64(seg, s):
    return np.repeat(np.asarray(s, np.float64), np.asarray(seg, np.int64), axis=-1)


def test_levels_merge(hml):
    """chains A and B (different chain ids) on one trace: after merge_levels(A, B) A holds the element-wise sum of the two
    dense expansions within E1 + E1', the counts add, the boundaries are the union; no relabelling anywhere"""
    T, K, seed = 80000, 4, 13
    x = ol.trace(T, K, 7)
    schemeA, schemeB = [("F", 20, 2)], [("M", 5, 0), ("F", 12, 1)]
    a, (segA, nA, a1, a2) = _levels_of(hml, x, K, seed, schemeA, chain=0)
    b, (segB, nB, b1, b2) = _levels_of(hml, x, K, seed, schemeB, chain=1)
    sweepsA = checker_sweeps(checker(K, seed, x, chain=0), schemeA)
    sweepsB = checker_sweeps(checker(K, seed, x, chain=1), schemeB)
    EA = lu.bounds(len(segA), nA, lu.max_abs_mean(sweepsA))
    EB = lu.bounds(len(segB), nB, lu.max_abs_mean(sweepsB))
    a.merge_levels(b)
    seg, n, s1, s2 = a.levels_rle()
    assert n == nA + nB == 22
    union = np.union1d(np.cumsum(segA) - segA, np.cumsum(segB) - segB).astype(np.int64)
    assert np.array_equal(np.cumsum(seg) - seg, union)
    err1 = np.max(np.abs(dense64(seg, s1) - (dense64(segA, a1) + dense64(segB, b1))))
    err2 = np.max(np.abs(dense64(seg, s2) - (dense64(segA, a2) + dense64(segB, b2))))
    print("merge: |S1 error| %.3g (bound %.3g), |S2 error| %.3g (bound %.3g)" % (err1, EA[0] + EB[0], err2, EA[1] + EB[1]))
    assert err1 <= EA[0] + EB[0] and err2 <= EA[1] + EB[1]
    # ... and the checker's two chains, accumulated together
    assert_levels(a, sweepsA + sweepsB, T, what="merged")
    # the source is unchanged, the destination records on
    assert np.array_equal(bits64(b.levels_rle()[2]), bits64(b1))
    a.iterate("F", 2, 1)
    a.sync()
    assert a.levels_rle()[1] == 24
    # other positions: refused
    c, _ = _levels_of(hml, x[:40000], K, seed, [("F", 4, 1)])
    with pytest.raises(hml.HmlError) as e:
        a.merge_levels(c)
    assert e.value.code == 1


@pytest.mark.parametrize("name", list(lu.EXACT_CASES))
def test_levels_double_sums_exactly(hml, name):
    """levels_rle() and levels_on_segments() against the numpy restatement of the device's additions (tests/levels_util.py:
    exact_cells, exact_merge, exact_scan, exact_on_segments), BIT FOR BIT: the order of the scan's additions is part of what
    the library computes.  The cases put M into every regime of the scan's tree (lu.EXACT_CASES; the range is asserted)."""
    kind, T, K, seed, chains, _ = lu.EXACT_CASES[name]
    x = lu.exact_case_trace(name)
    sweeps = [checker_sweeps(checker(K, seed, x, chain=ch), scheme) for ch, scheme in chains]
    cells = lu.exact_case_cells(name, sweeps)
    pos, want = lu.exact_rle(cells)
    gs = [_levels_of(hml, x, K, seed, scheme, chain=ch)[0] for ch, scheme in chains]
    for other in gs[1:]:
        gs[0].merge_levels(other)
    seg, n, s1, s2 = gs[0].levels_rle()
    assert n == sum(len(s) for s in sweeps)
    assert np.array_equal(seg.astype(np.int64), np.diff(np.append(pos, T))), name
    cuts = lu.exact_case_cuts(name, cells)
    o1, o2 = gs[0].levels_on_segments(cuts)
    want_on = lu.exact_on_segments(cells, cuts)
    got = [(s1[0], want[0]), (s2[0], want[1]), (o1[0], want_on[0]), (o2[0], want_on[1])]
    differing = [int(np.sum(bits64(a) != bits64(b))) for a, b in got]
    print("%s: M=%d, %d cuts; entries with other bits: sum %d, sum_sq %d, on segments %d / %d" % ((name, len(seg), len(cuts)) + tuple(differing)))
    assert differing == [0, 0, 0, 0], (name, differing)


def test_levels_are_label_invariant(hml):
    """the point of the feature: the same sweep with the states renamed - parameters, rows and columns of A and pi permuted
    alike, static blocks, one sweep with probes - against the checker fed the same permuted parameters"""
    T, K, seed = 60000, 4, 9
    x = ol.trace(T, K, 7)
    perm = np.array([2, 0, 3, 1])
    for renamed in (False, True):
        o = checker(K, seed, x)
        g = gpu_chain(hml, K, seed, x)
        o.token("F")
        g.sample_prior()
        g._pending_prior = False
        o.iterate("F", 10, 0)
        g.iterate("F", 10, 0)
        mv, (A, pi) = g.theta().reshape(K, 2), g.transitions()
        if renamed:
            mv, A, pi = mv[perm], A[np.ix_(perm, perm)], pi[perm]
        o.set_params(mv.reshape(-1), A, pi)
        g.set_parameters(mv.reshape(-1), A, pi)
        o.token("S")
        g.set_static_blocks()
        o.set_probes(True)
        g.enable_probes(True)
        o.iterate("F", 1, 0)
        g.iterate("F", 1, 1)
        g.sync()
        assert np.array_equal(o.states(), g.states())
        sweeps = [(o.blocks().copy(), o.states().copy(), o.theta()[0::2].copy())]
        assert_levels(g, sweeps, T, what="renamed" if renamed else "original")


def test_levels_dense_device(hml):
    """hml_levels_dense_device into a torch buffer = levels_mean_sd expanded by the segment lengths, as float32, exactly"""
    import torch
    T, P, D = 50000, 2, 2
    x = np.stack([ol.trace(T, P, 9 + d) for d in range(D)], axis=1).reshape(-1)
    g = gpu_chain(hml, P ** D, 6, x, D=D, P=P)
    g.sample_prior()
    g.iterate("F", 21, 2)
    g.sync()
    seg, n, s1, s2 = g.levels_rle()
    assert n == 10 and len(seg) > 1
    out = torch.full((2 * D, T), -7.0, dtype=torch.float32, device="cuda:0")
    g.levels_dense_device(out.data_ptr())
    got = out.cpu().numpy()
    mean, sd = hml.levels_mean_sd(n, s1, s2)
    for d in range(D):
        assert np.array_equal(got[2 * d].view(np.uint32), np.repeat(mean[d], seg.astype(np.int64)).view(np.uint32)), d
        assert np.array_equal(got[2 * d + 1].view(np.uint32), np.repeat(sd[d], seg.astype(np.int64)).view(np.uint32)), d
    assert np.all(sd >= 0) and np.any(sd > 0)


@pytest.mark.parametrize("name", ["scale_2p40", "offset_1000", "tiny_2"])
def test_levels_on_hostile_inputs(hml, name):
    """data scaled by 2^40, data shifted by 1000, a trace of two positions: the same bound"""
    fn, K, scheme = hi.INPUTS[name]
    x = hi.data(name)
    run_case(hml, x, K, hi.SEED[name], scheme, x.size, what=name)


def test_levels_off_by_default(hml):
    T, K = 50000, 3
    x = ol.trace(T, K, 7)
    g = gpu_chain(hml, K, 5, x, levels=False)
    g.profile_enable(2)
    g.sample_prior()
    g.iterate("F", 10, 1)
    g.sync()
    assert g.recorded_sweeps() == 10
    assert g.profile_get("marginals")[1] == 10 and g.profile_get("levels")[1] == 0
    with pytest.raises(hml.HmlError) as e:
        g.levels_rle()
    assert e.value.code == 1 and "hml_set_level_recording" in str(e.value)
    # turned on later: recorded from then on; turned off again: what was accumulated stays
    g.set_level_recording(True)
    g.iterate("F", 4, 2)
    g.set_level_recording(False)
    g.iterate("F", 4, 1)
    g.sync()
    assert g.levels_rle()[1] == 2 and g.profile_get("levels")[1] == 2 and g.recorded_sweeps() == 16

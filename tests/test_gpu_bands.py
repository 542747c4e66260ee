"""Level bands per position on the GPU (hml_k_bands.h behind hml_set_level_bands / hml_bands_rle / hml_bands_dense_device /
hml_bands_call / hml_bands_merge).  The expected counts come from the CPU CHECKER - its blocks, states and theta after every
recorded sweep, stepped one sweep per call - accumulated by tests/bands_util.py; never from the product.  Everything is
integers: every comparison is exact.  tests/test_bands_cpu.py shows on the checker alone that every case of
tests/bands_cases.py has something to find."""
import math

import numpy as np
import pytest

from tests import bands_cases as bc
from tests import bands_util as bu
from tests import hostile_inputs as hi
from tests import oracle_lib as ol

pytestmark = pytest.mark.gpu


def gpu_chain(hml, c, chain=0, options=(), edges="case", attach=None, seed=None, trace=None):
    g = hml.Chain(device=0, seed=c["seed"] if seed is None else seed, chain_id=chain)
    for name, value in options:
        g.set_option(name, value)
    if c["compat"]:
        g.set_option("compat", 1)
    if attach is not None:
        g.attach(attach)
    else:
        if c["D"] > 1:
            g.set_dimensions(c["D"], c["P"])
        x = trace if trace is not None else c["trace"]
        g.load(x() if callable(x) else x)
    g.set_model(c["K"], g.autoprior(0.2, 0.9))
    if edges is not None:
        g.set_level_bands(c["edges"] if isinstance(edges, str) else edges)
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


def gpu_run(g, scheme):
    for tok in scheme:
        gpu_token(g, tok)
    g.sync()
    return g


def shape_of(c):
    return c["D"], (c["P"] if c["D"] > 1 else c["K"]), len(c["edges"]) + 1


def assert_bands(hml, g, sweeps, c, what="", edges=None):
    """bands_rle() of the GPU chain against the helper fed the checker's sweeps, exactly; returns (length, counts, N)"""
    D, P, nb = shape_of(c)
    edges = c["edges"] if edges is None else edges
    nb = len(edges) + 1
    counts, boundary, N = bu.accumulate(sweeps, c["T"], edges, D=D, P=P)
    length, want = bu.rle(counts, boundary)
    seg, cnt, n = g.bands_rle()
    print("%s: %d band segments, %d level segments, N = %d" % (what, len(length), bu.level_segments(sweeps, c["T"]), N))
    assert n == N, (what, n, N)
    assert cnt.shape == (len(length), D * nb) and cnt.dtype == np.int32
    assert np.array_equal(seg.astype(np.int64), length), what
    assert np.array_equal(cnt.astype(np.int64), want), what
    assert np.array_equal(hml.bands_exceedance(cnt, len(edges), D), bu.exceedance(want, len(edges), D)), what
    return length, want, N


def run_case(hml, c, what="", options=(), sweeps=None):
    """blocks, states and theta bits equal to the checker's first, then the bands"""
    o = bc.checker(c)
    try:
        if sweeps is None:
            sweeps = bc.checker_sweeps(o, c["scheme"])
        else:                                   # (the shared sweeps of a named case: bring the checker to the end of the scheme)
            bc.checker_sweeps(o, c["scheme"])
        g = gpu_run(gpu_chain(hml, c, options=options), c["scheme"])
        assert np.array_equal(o.blocks(), g.blocks()) and np.array_equal(o.states(), g.states()), what
        assert np.array_equal(o.theta().view(np.uint32), g.theta().view(np.uint32)), what
    finally:
        o.close()
    return g, sweeps, assert_bands(hml, g, sweeps, c, what=what)


@pytest.mark.parametrize("name", sorted(bc.CASES))
def test_bands_match_checker(hml, name):
    """K = 3 ... 40 (sweep_k, sweep_wide), read-depth data, `-s C 2 2`, the reference-compatible mode, mixed schemes"""
    c = bc.CASES[name]
    g, sweeps, (length, want, N) = run_case(hml, c, what=name)
    assert np.array_equal(g.level_bands(), np.asarray(c["edges"], np.float32))
    assert len(length) < bu.level_segments(sweeps, c["T"])      # coarser than the levels' segments (test_bands_cpu.py)


def test_bands_thinning_on_one_chain(hml):
    """thinning 1, 2, 3 and 7 in the tokens of one chain"""
    c = dict(bc.CASES["k3"], T=50000, trace=lambda: ol.trace(50000, 3, 7), seed=11,
             scheme=[("F", 6, 1), ("F", 8, 2), ("F", 9, 3), ("F", 15, 7)])
    g, sweeps, (length, want, N) = run_case(hml, c, what="thinning")
    assert N == 6 + 4 + 3 + 2


def test_level_on_an_edge_lands_in_the_band_above(hml):
    """the float mean of one state after recorded sweep n, taken from the checker, is the edge: that sweep's level equals the
    edge and belongs to the band above it"""
    base = dict(bc.CASES["k3"], T=50000, trace=lambda: ol.trace(50000, 3, 7), seed=23, scheme=[("F", 12, 2)])
    o = bc.checker(base)
    sweeps = bc.checker_sweeps(o, base["scheme"])
    o.close()
    n = 3
    starts, states, mean = sweeps[n]
    s = int(states[len(states) // 2])
    edge = np.float32(mean[s])
    c = dict(base, edges=(float(edge),))
    assert np.float32(c["edges"][0]) == edge
    # on the checker's data: the equality occurs in sweep n, under a run of that state, and the helper puts it in band 1
    pos, bands = bu.sweep_bands(sweeps[n], c["edges"], 1, 3)
    assert np.any(states == s) and mean[s] == edge and np.all(bands[0][bu.lu.run_starts(starts, states)[1] == s] == 1)
    assert bu.band_of(c["edges"], np.nextafter(edge, np.float32(-np.inf))) == 0
    g, _, (length, want, N) = run_case(hml, c, what="level on an edge")
    t = int(starts[len(states) // 2])
    counts, _, _ = bu.accumulate([sweeps[n]], c["T"], c["edges"])
    assert counts[1, t] == 1 and counts[0, t] == 0


def test_bands_iterate_many_equals_iterate_bit_for_bit(hml):
    """three chains attached to one trace through hml_iterate_many (the band kernel runs per chain behind the batch's
    parameter kernels): each chain's bands are those of the same chain alone under hml_iterate - and the checker's"""
    c = dict(bc.CASES["k5"], seed=21, scheme=[("F", 12, 0), ("F", 18, 3)])
    alone = []
    for k in range(3):
        g = gpu_run(gpu_chain(hml, c, chain=k), c["scheme"])
        alone.append(g.bands_rle())
        g.close()
    first = gpu_chain(hml, c, chain=0)
    chains = [first] + [gpu_chain(hml, c, chain=k, attach=first) for k in (1, 2)]
    for g in chains:
        g.sample_prior()
        g._pending_prior = False
    for m, n, t in c["scheme"]:
        hml.iterate_many(chains, m, n, t)
    for k, g in enumerate(chains):
        g.sync()
        seg, cnt, n = g.bands_rle()
        assert n == alone[k][2] == 6
        assert np.array_equal(seg, alone[k][0]) and np.array_equal(cnt, alone[k][1]), k
        o = bc.checker(c, chain=k)
        assert_bands(hml, g, bc.checker_sweeps(o, c["scheme"]), c, what="iterate_many chain %d" % k)
        o.close()


def test_bands_survive_buffer_growth(hml):
    """a block capacity far below what the sweeps need: the chain halts, grows and runs the sweeps again - every recorded
    sweep is counted once"""
    c = dict(bc.CASES["k3"], seed=8, scheme=[("M", 4, 1), ("F", 16, 2)])
    g0 = gpu_run(gpu_chain(hml, c), c["scheme"])
    g1 = gpu_run(gpu_chain(hml, c, options=(("max_blocks", 64),)), c["scheme"])
    assert g0.stats()["buffer_growths"] == 0 and g1.stats()["buffer_growths"] > 0
    ref, got = g0.bands_rle(), g1.bands_rle()
    assert got[2] == ref[2] == 12 and np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
    o = bc.checker(c)
    assert_bands(hml, g1, bc.checker_sweeps(o, c["scheme"]), c, what="max_blocks 64")
    o.close()


def test_bands_reproducible(hml):
    c = dict(bc.CASES["k5"], T=150000, trace=lambda: ol.trace(150000, 5, 7), seed=3, scheme=[("F", 20, 2)])
    runs = [gpu_run(gpu_chain(hml, c), c["scheme"]).bands_rle() for _ in range(2)]
    assert runs[0][2] == runs[1][2] == 10
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])


def test_bands_merge(hml):
    """two chains of different seeds merged = the helper fed both chains' sweeps; the destination records on; mismatched
    edges, T or D are refused"""
    c = dict(bc.CASES["k4_mixed"], T=80000, trace=lambda: ol.trace(80000, 4, 7))
    cA = dict(c, seed=13, scheme=[("F", 20, 2)])
    cB = dict(c, seed=14, scheme=[("M", 5, 0), ("F", 12, 1)])
    a = gpu_run(gpu_chain(hml, cA), cA["scheme"])
    b = gpu_run(gpu_chain(hml, cB, chain=1), cB["scheme"])
    oA, oB = bc.checker(cA), bc.checker(cB, chain=1)
    sweepsA, sweepsB = bc.checker_sweeps(oA, cA["scheme"]), bc.checker_sweeps(oB, cB["scheme"])
    before = b.bands_rle()
    a.merge_bands(b)
    length, want, N = assert_bands(hml, a, sweepsA + sweepsB, c, what="merged")
    assert N == 22
    after = b.bands_rle()                                   # the source is unchanged
    assert after[2] == before[2] and np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1])
    a.iterate("F", 4, 2)                                    # the destination records on
    a.sync()
    more = []
    for i in range(4):
        oA.iterate("F", 1, 0)
        if i % 2 == 1:
            more.append((oA.blocks().copy(), oA.states().copy(), oA.theta()[0::2].copy()))
    assert_bands(hml, a, sweepsA + sweepsB + more, c, what="merged, then recorded on")
    # a destination that was never asked gets its buffers and the source's edges
    fresh = gpu_chain(hml, cA, edges=None)
    fresh.merge_bands(b)
    assert_bands(hml, fresh, sweepsB, c, what="merged into a fresh context")
    oA.close()
    oB.close()
    # refused: other edges (one bit), other positions, other dimensions
    other = np.asarray(c["edges"], np.float32).copy()
    other[0] = np.nextafter(other[0], np.float32(0))
    mv = bc.CASES["mv_c22"]
    for bad in (gpu_run(gpu_chain(hml, cA, edges=other), [("F", 2, 1)]),
                gpu_run(gpu_chain(hml, dict(cA, T=40000), trace=lambda: ol.trace(40000, 4, 7)), [("F", 2, 1)]),
                gpu_run(gpu_chain(hml, dict(mv, trace=lambda: np.stack([ol.trace(80000, 2, 9 + d) for d in range(2)], axis=1).reshape(-1)),
                                  edges=c["edges"]), [("F", 2, 1)])):
        with pytest.raises(hml.HmlError) as e:
            a.merge_bands(bad)
        assert e.value.code == 1
    assert a.bands_rle()[2] == 24


def test_edges_cannot_change_once_recorded(hml):
    c = dict(bc.CASES["k3"], T=50000, trace=lambda: ol.trace(50000, 3, 7))
    g = gpu_chain(hml, c, edges=(-0.25, 0.25))
    g.set_level_bands(c["edges"])                           # before a recorded sweep: free
    gpu_run(g, [("F", 4, 0), ("F", 4, 2)])
    g.set_level_bands(c["edges"])                           # the same bits: fine
    for bad in ((-0.5, 0.25), (-0.5,), (0.5, -0.5), (0.0, 0.0), (float("nan"),), (float("inf"),), tuple(range(32))):
        with pytest.raises(hml.HmlError) as e:
            g.set_level_bands(bad)
        assert e.value.code == 1, bad
    assert g.bands_rle()[2] == 2 and np.array_equal(g.level_bands(), np.asarray(c["edges"], np.float32))


def test_bands_are_label_invariant(hml):
    """the same sweep with the states renamed - parameters, rows and columns of A and pi permuted alike, static blocks, one
    sweep with probes: identical band counts, while the state marginals differ"""
    c = dict(bc.CASES["k4_mixed"], T=60000, trace=lambda: ol.trace(60000, 4, 7), seed=9)
    K = 4
    perm = np.array([2, 0, 3, 1])
    seen = []
    for renamed in (False, True):
        o = bc.checker(c)
        g = gpu_chain(hml, c)
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
        assert_bands(hml, g, sweeps, c, what="renamed" if renamed else "original")
        seen.append((g.bands_rle(), g.marginals_rle()))
        o.close()
    (b0, m0), (b1, m1) = seen
    assert np.array_equal(b0[0], b1[0]) and np.array_equal(b0[1], b1[1])
    assert not (np.array_equal(m0[0], m1[0]) and np.array_equal(m0[1], m1[1]))


def test_bands_dense_device(hml):
    """hml_bands_dense_device, plain and cumulative, at T = 100003 (a span tail) against the helper's dense counts"""
    import torch
    T = 100003
    c = dict(bc.CASES["k3"], T=T, trace=lambda: ol.trace(T, 3, 7), seed=6, scheme=[("F", 21, 2)])
    g, sweeps, (length, want, N) = run_case(hml, c, what="dense")
    counts, boundary, _ = bu.accumulate(sweeps, T, c["edges"])
    out = torch.full((3, T), -7, dtype=torch.int32, device="cuda:0")
    g.bands_dense_device(out.data_ptr())
    assert np.array_equal(out.cpu().numpy().astype(np.int64), counts)
    g.bands_dense_device(out.data_ptr(), cumulative=True)
    got = out.cpu().numpy().astype(np.int64)
    assert np.array_equal(got, bu.cumulative(counts, 1, 3))
    assert N == 10 and np.all(got[0] == N)


@pytest.mark.parametrize("name", bc.RANK_CASES)
def test_bands_call(hml, name):
    """rank 0, 1, ceil(N / 2) and N against the helper, D = 1 and D = 2; rank N + 1 is refused"""
    c = bc.CASES[name]
    D, P, nb = shape_of(c)
    g, sweeps, (length, want, N) = run_case(hml, c, what=name, sweeps=bc.sweeps_of(name))
    for rank in (0, 1, int(math.ceil(N / 2)), N):
        run_len, run_band = g.bands_call(rank)
        want_len, want_band = bu.call(want, length, rank, D, nb)
        assert run_band.shape == (D, len(want_len)), (name, rank)
        assert np.array_equal(run_len.astype(np.int64), want_len) and np.array_equal(run_band, want_band), (name, rank)
    with pytest.raises(hml.HmlError) as e:
        g.bands_call(N + 1)
    assert e.value.code == 1


HOSTILE = hi.family("ties", "spikes", "tiny") + ["scale_2p40", "offset_1000"]


@pytest.mark.parametrize("name", HOSTILE)
def test_bands_on_hostile_inputs(hml, name):
    """integer data with exact ties, spikes, traces of 2 to 65 positions, scaled and shifted data; edges at the data's
    quartiles (numpy, as float32; equal quartiles of tied data count once)"""
    fn, K, scheme = hi.INPUTS[name]
    x = hi.data(name)
    edges = np.unique(np.quantile(x.astype(np.float64), [0.25, 0.5, 0.75]).astype(np.float32))
    assert np.all(np.isfinite(edges)) and len(edges) >= 1
    c = dict(T=x.size, K=K, seed=hi.SEED[name], scheme=scheme, trace=x, D=1, P=None, compat=False, env={}, edges=tuple(float(e) for e in edges))
    run_case(hml, c, what=name)


def test_bands_off_by_default(hml):
    """no bands set: no launch, the read-out refuses; with bands on, everything else is bit for bit what it is with bands off"""
    c = dict(bc.CASES["k3"], T=50000, trace=lambda: ol.trace(50000, 3, 7), seed=5, scheme=[("F", 10, 1)])
    kept = []
    for edges in (None, "case"):
        g = gpu_chain(hml, c, edges=edges)
        g.set_level_recording(True)
        g.profile_enable(2)
        gpu_run(g, c["scheme"])
        assert g.recorded_sweeps() == 10 and g.profile_get("marginals")[1] == 10
        assert g.profile_get("bands")[1] == (0 if edges is None else 10)
        if edges is None:
            with pytest.raises(hml.HmlError) as e:
                g.bands_rle()
            assert e.value.code == 1 and "hml_set_level_bands" in str(e.value)
        kept.append((g.blocks(), g.states(), g.theta().view(np.uint32), g.marginals_rle(), g.levels_rle()))
    a, b = kept
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert np.array_equal(a[3][0], b[3][0]) and np.array_equal(a[3][1], b[3][1])
    assert a[4][1] == b[4][1] and np.array_equal(a[4][0], b[4][0])
    assert np.array_equal(a[4][2].view(np.uint64), b[4][2].view(np.uint64)) and np.array_equal(a[4][3].view(np.uint64), b[4][3].view(np.uint64))
    # asked, nothing recorded: one segment of zeros with N = 0; turned off: what was accumulated stays
    g = gpu_chain(hml, c)
    gpu_run(g, [("F", 4, 0)])
    seg, cnt, n = g.bands_rle()
    assert n == 0 and list(seg) == [c["T"]] and not cnt.any()
    g.iterate("F", 4, 2)
    g.set_level_bands(())
    g.iterate("F", 4, 1)
    g.sync()
    assert g.bands_rle()[2] == 2 and g.recorded_sweeps() == 6

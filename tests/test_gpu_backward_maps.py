"""The backward pass keeps a map [K] -> [K] per row in one 64-bit word: a byte per entry up to 8 states, composed by a byte
permute (hammlet_amd/csrc/hml_maps.h), 4 bits per entry beyond.  The packed words never leave the device, so what shows here
is the chain: every case runs against the device-mode checker, bit for bit - lengths on both sides of a backward chunk (64
rows) and a reduction chunk (256), with a last row alone in its chunk (the broadcast map); both partitions of the one-workgroup
chain (up to 4096 chunk maps: four per thread in registers; beyond: a loop); the repair step, which computes maps again; a
chain whose blocks outgrow its buffers; the two-level chain; and chains batched into one launch (two rows per lane)."""
import numpy as np
import pytest

from tests import oracle_lib as ol
from tests.test_gpu_parity import bits, compare_state, make_pair, run_both, setup_model

pytestmark = pytest.mark.gpu

LENGTHS = [1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1025]


def set_up(o, g, x, K):
    """the automatic prior - except for a single observation, whose data variance of zero the prior's rule refuses (checker
    and library alike): both sides are given one fixed prior instead (as tests/test_gpu_head_loads.py does)"""
    if len(x) > 1:
        return setup_model(o, g, K)
    p = np.array([2.0, 0.1, float(x[0]), 1.0], np.float32)
    o.set_prior(p)
    o.init_model()
    g.set_model(K, p, 0.5, 0.5, 0.5, True)
    return p


def run_chain(hml, T, K, scheme):
    x, o, g = make_pair(hml, T, K, 7, 42, weight_mult=1e9)
    set_up(o, g, x, K)
    g._pending_prior = True
    o.set_record(marginals=True)
    run_both(o, g, scheme)
    return o, g


def check(hml, o, g, what):
    compare_state(o, g, what=what)       # blocks, states, theta, A, pi
    seg, cnt = g.marginals_rle()
    assert hml.marginals_text(seg, cnt) == o.text("marginals")


@pytest.mark.parametrize("K", [2, 5, 8, 9, 10])
@pytest.mark.parametrize("T", LENGTHS)
def test_every_position_a_block(hml, T, K):
    o, g = run_chain(hml, T, K, [("F", 6, 1)])
    assert len(g.blocks()) == T + 1, "every position a block"   # (the starts and the end marker)
    check(hml, o, g, "T = %d, %d states" % (T, K))


@pytest.mark.parametrize("T", [4096 * 64 - 1, 4096 * 64, 4096 * 64 + 1])
def test_both_partitions_of_the_chain(hml, T):
    """4096 chunk maps (four per thread, kept in registers) and 4097 (a loop over the thread's maps)"""
    o, g = run_chain(hml, T, 5, [("F", 2, 1)])
    assert len(g.blocks()) == T + 1
    check(hml, o, g, "T = %d" % T)


@pytest.mark.parametrize("K", [4, 8])
def test_repair_computes_byte_maps_again(hml, K):
    """The twin states of test_forward_repair_paths_on_twin_states (tests/test_gpu_parity.py) in a model of K states: two
    states with the same emission parameters and sticky transitions forget their start slowly, the forward chunks fail
    their verification, and the repair step writes the maps of those chunks."""
    T = 1_000_000
    x = ol.trace(T, 3, 1)
    xx, o, g = make_pair(hml, T, K, 0, 1, x=x)
    setup_model(o, g, K)
    o.token("F")
    g.sample_prior()
    mv = np.zeros(2 * K, np.float32)
    mv[0::2] = [-1.0, 0.5, 0.5] + [3.0 + s for s in range(K - 3)]    # states 1 and 2 are twins; the others lie off the trace
    mv[1::2] = 0.04
    A = np.zeros((K, K), np.float64)
    A[:3, :3] = [[0.999, 0.0005, 0.0005], [0.0005, 0.9994, 0.0001], [0.0005, 0.0001, 0.9994]]   # that test's matrix ...
    A[:3, 3:] = 1e-6                                                                            # ... and hardly a way to the others
    A[3:, :] = 0.001 / (K - 1)
    A[np.arange(K), np.arange(K)] = 0.0
    A[np.arange(K), np.arange(K)] = np.where(np.arange(K) < 3, [0.999, 0.9994, 0.9994] + [0.0] * (K - 3), 0.999) - np.where(np.arange(K) < 3, (K - 3) * 1e-6, 0.0)
    A = A.astype(np.float32)
    pi = np.array([0.2, 0.5, 0.3] + [0.0] * (K - 3), np.float32) * np.float32(0.999) + np.float32(0.001 / K)
    o.set_params(mv, A, pi)
    g.set_parameters(mv, A, pi)
    s0 = g.stats()
    o.iterate("F", 1, 0)
    g.iterate("F", 1, 0)
    g.sync()
    s1 = g.stats()
    assert s1["forward_refits"] > s0["forward_refits"]
    assert np.array_equal(o.blocks(), g.blocks())
    assert np.array_equal(o.states(), g.states())
    o.iterate("F", 4, 0)
    g.iterate("F", 4, 0)
    g.sync()
    compare_state(o, g, what="%d states" % K)


def test_blocks_that_outgrow_the_buffers(hml):
    """Option max_blocks = 64 on a trace that needs hundreds and, after a prior re-draw, thousands of blocks (as
    test_block_capacity_grows_without_changing_the_chain): the sweep behind the enumeration that halted runs on buffers far
    smaller than its grids assume."""
    K, T = 5, 300_000
    x = ol.trace(T, K, 12)
    o = ol.OracleChain(K=K, seed=9, chain=0, rng=ol.RNG_CTR, math=ol.MATH_DEV, reduce=ol.REDUCE_DEV)
    o.load(x)
    g = hml.Chain(device=0, seed=9, chain_id=0)
    g.set_option("max_blocks", 64)
    g.load(x)
    setup_model(o, g, K)
    o.token("F")
    g.sample_prior()
    o.set_record(marginals=True)
    for method, iters, thin in (("F", 10, 0), ("F", 4, 2), ("P", 0, 0), ("F", 6, 3)):
        if method == "P":
            o.token("P")
            o.token("F")
            g.sample_prior()
            continue
        o.iterate(method, iters, thin)
        g.iterate(method, iters, thin)
        g.sync()
        compare_state(o, g, what="%s %d %d" % (method, iters, thin))
    st = g.stats()
    assert st["buffer_growths"] >= 1 and 64 < st["block_capacity"] < T
    seg, cnt = g.marginals_rle()
    assert hml.marginals_text(seg, cnt) == o.text("marginals")
    g.close()


@pytest.mark.parametrize("K", [5, 10])
def test_two_level_chain(hml, monkeypatch, K):
    """forced the way tests/test_gpu_sweep_paths.py ("dense_separate") forces it: every sweep counts as one of many blocks, the
    fused trellis path is off - super maps of 64 chunks, the chain over those, entries from the suffix maps"""
    monkeypatch.setenv("HML_DENSE_MIN_BLOCKS", "1")
    monkeypatch.setenv("HML_TRELLIS_FUSED", "0")
    T = 64 * 64 * 3 + 65    # three full super-chunks, a fourth of two chunks, the last of one row
    o, g = run_chain(hml, T, K, [("F", 4, 1)])
    assert len(g.blocks()) == T + 1
    check(hml, o, g, "two-level chain, %d states" % K)


@pytest.mark.parametrize("attached", [False, True])
def test_batched_chains(hml, attached):
    """hml_iterate_many over three chains (hml_k_many.h: two rows per lane in the maps kernel), on constructions of their own and
    on a shared one: each is the chain the checker runs alone"""
    K, T = 5, 100_000
    x = ol.trace(T, K, 12)
    pairs = []
    for chain in range(3):
        o = ol.OracleChain(K=K, seed=9, chain=chain, rng=ol.RNG_CTR, math=ol.MATH_DEV, reduce=ol.REDUCE_DEV)
        o.load(x)
        g = hml.Chain(device=0, seed=9, chain_id=chain)
        if attached and chain > 0:
            g.attach(pairs[0][1])
        else:
            g.load(x)
        setup_model(o, g, K)
        o.token("F")
        g.sample_prior()
        o.set_record(marginals=True)
        pairs.append((o, g))
    gs = [g for _, g in pairs]
    for iters, thin in ((10, 0), (6, 2)):
        for o, _ in pairs:
            o.iterate("F", iters, thin)
        hml.iterate_many(gs, "F", iters, thin)
        for chain, (o, g) in enumerate(pairs):
            g.sync()
            compare_state(o, g, what="batched chain %d" % chain)
    for o, g in pairs:
        seg, cnt = g.marginals_rle()
        assert hml.marginals_text(seg, cnt) == o.text("marginals")
    assert not np.array_equal(bits(gs[0].theta()), bits(gs[1].theta()))
    for g in reversed(gs):
        g.close()

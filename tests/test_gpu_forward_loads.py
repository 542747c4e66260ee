"""The forward filter addresses the emission terms of a FULL batch by plane (hml_fwd_run, hml_k_forward.h): where every lane
of a wavefront has a whole batch ahead of it, inside one column of its chunk and from the same row on, the loads go out from
one per-lane address and wave-uniform plane offsets, without a predicate; every other batch - the tail of a chunk, a warm-up
window clipped at block 0, a warm-up that is no multiple of the batch, chunks shorter than a batch - takes the general
form.  Which form a batch takes must not show: chains whose every position is a block (weights scaled by 1e9, so B = T) at
lengths on both sides of everything the choice tests for, for 2, 5, 7 states (the transition matrix in registers, batches
of 4 up to 6 states and of 2 beyond) and 8, 10 states (the matrix in LDS, batches of 2), warm-ups around the batch size,
chunks of 4 and of 8, and chains batched into one launch - against the device-mode checker, bit for bit.  The checker's
rows do not depend on the warm-up: it runs the sequential recursion."""
import numpy as np
import pytest

from tests import oracle_lib as ol
from tests.test_gpu_parity import bits, compare_state, make_pair, run_both, setup_model

gpu = pytest.mark.gpu

# one batch, one chunk | the first unclipped warm-up window at W = 12 | one wavefront of chunks | one workgroup of chunks,
# with a last chunk of 1, 3 or 4 blocks
LENGTHS = [1, 3, 4, 5, 7, 8, 12, 13, 16, 17, 255, 256, 257, 1023, 1024, 1025, 1027]
STATES = [2, 5, 7, 8, 10]
SCHEME = [("F", 3, 0), ("F", 1, 1), ("F", 2, 0)]   # a few sweeps, one of them recorded
WARMUPS = [0, 3, 4, 6, 12, 13]


def set_up(o, g, x, K):
    """The automatic prior - except for a single observation: its data variance is zero, which the prior's rule refuses
    (checker and library alike), so both sides are given one fixed prior instead.  g = None: the checker alone."""
    if len(x) > 1:
        if g is not None:
            return setup_model(o, g, K)
        p = o.autoprior()
        o.init_model()
        return p
    p = np.array([2.0, 0.1, float(x[0]), 1.0], np.float32)
    o.set_prior(p)
    o.init_model()
    if g is not None:
        g.set_model(K, p, 0.5, 0.5, 0.5, True)
    return p


def run_chain(hml, T, K):
    """checker and chain after the scheme, and the chain's statistics before and after it"""
    x, o, g = make_pair(hml, T, K, 7, 42, weight_mult=1e9)
    set_up(o, g, x, K)
    g._pending_prior = True
    o.set_record(marginals=True)
    s0 = g.stats()
    run_both(o, g, SCHEME)
    return o, g, s0, g.stats()


def check(hml, o, g, T, what):
    assert len(g.blocks()) == T + 1, "every position a block"   # (the starts and the end marker)
    compare_state(o, g, what=what)                               # blocks, states, theta, A, pi
    seg, cnt = g.marginals_rle()
    assert hml.marginals_text(seg, cnt) == o.text("marginals")


@pytest.mark.parametrize("K", STATES)
def test_checker_runs_the_ordinary_chain_on_these_inputs(oracle, K):
    """No GPU: on every input of this file the checker runs its ordinary chain - every position a block, every sweep of the
    scheme carried out, finite parameters and a proper transition matrix at the end - so a comparison with it says something."""
    for T in LENGTHS + [4099]:
        x = ol.trace(T, K if K in ol.LEVELS else 6, 7)
        o = ol.OracleChain(K=K, seed=42, chain=0, rng=ol.RNG_CTR, math=ol.MATH_DEV, reduce=ol.REDUCE_DEV, weight_mult=1e9)
        o.load(x)
        set_up(o, None, x, K)
        o.set_record(marginals=True)
        for m, n, t in SCHEME:
            o.iterate(m, n, t)
        assert len(o.blocks()) == T + 1, (T, K)
        assert o.total_blocks() == T * sum(n for _, n, _ in SCHEME), (T, K)
        assert len(o.states()) == T and 0 <= o.states().min() and o.states().max() < K
        A, pi = o.transitions()
        assert np.all(np.isfinite(o.theta())) and np.all(np.isfinite(A)) and np.all(np.isfinite(pi)), (T, K)
        assert np.all(np.asarray(A) >= 0.0) and np.allclose(np.asarray(A).reshape(K, K).sum(axis=1), 1.0, atol=1e-5), (T, K)
        assert o.text("marginals")
        o.close()


@gpu
@pytest.mark.parametrize("K", STATES)
@pytest.mark.parametrize("T", LENGTHS)
def test_every_position_a_block(hml, T, K):
    o, g, _, _ = run_chain(hml, T, K)
    check(hml, o, g, T, "T = %d, %d states" % (T, K))
    g.close()


@gpu
@pytest.mark.parametrize("K", [5, 7, 8])
@pytest.mark.parametrize("T", [17, 257, 1027])
@pytest.mark.parametrize("W", WARMUPS)
def test_warm_ups_around_the_batch_size(hml, monkeypatch, W, T, K):
    """HML_FWD_WARMUP: where a chain's warm-up starts and its floor.  12 is a multiple of both batch sizes, 6 of one, 13 and 3
    of neither (every warm-up batch starts at a row from which a batch of 4 leaves the chunk's column), 4 is one batch, 0
    none.  After 0 and 3 rows the filter has not forgotten its start: the verification fails and the repair step runs the
    chunks again, after longer warm-ups, through the same hml_fwd_run."""
    monkeypatch.setenv("HML_FWD_WARMUP", str(W))
    o, g, s0, s1 = run_chain(hml, T, K)
    print("W = %d, T = %d, K = %d: refits %d, serial %d, warm-up %d -> %d" % (
        W, T, K, s1["forward_refits"] - s0["forward_refits"], s1["forward_serial"] - s0["forward_serial"],
        s0["forward_warmup"], s1["forward_warmup"]))
    check(hml, o, g, T, "warm-up %d, T = %d, %d states" % (W, T, K))
    if W in (0, 3):
        assert s1["forward_refits"] > s0["forward_refits"], "the repair step did not run"
    g.close()


@gpu
@pytest.mark.parametrize("K", [5, 8])
@pytest.mark.parametrize("T", [1025, 4099])
def test_chunks_of_eight(hml, monkeypatch, T, K):
    """HML_MID_MIN_BLOCKS = 1: from the second sweep on (the first has no block count to go by) the chunks are 8 blocks long -
    two batches of 4 to a column, four of 2 - in a layout of their own.  No statistic of a chain tells which geometry a sweep
    ran under (same kernels, same launches: tests/test_gpu_sweep_paths.py); that the plan takes the mid geometry from a block
    count of at least mid_min_blocks on, below the dense threshold, is what tests/test_sweep_plan_cpu.py holds on the CPU.
    Both lengths are no multiple of 8 either: the last chunk is 1 and 3 blocks long."""
    monkeypatch.setenv("HML_MID_MIN_BLOCKS", "1")
    o, g, _, _ = run_chain(hml, T, K)
    check(hml, o, g, T, "chunks of 8, T = %d, %d states" % (T, K))
    g.close()


def lone_chain(hml, x, K, chain):
    g = hml.Chain(device=0, seed=9, chain_id=chain)
    try:
        g.load(x)
        g.scale_weights(1e9)
        g.set_model(K, g.autoprior(0.2, 0.9))
        g.sample_prior()
        for m, n, t in SCHEME:
            g.iterate(m, n, t)
        g.sync()
        A, pi = g.transitions()
        return g.blocks().copy(), g.states().copy(), bits(g.theta()).copy(), bits(A).copy(), bits(pi).copy(), hml.marginals_text(*g.marginals_rle())
    finally:
        g.close()


@gpu
def test_two_attached_chains_in_one_launch(hml):
    """hml_m_forward runs the same hml_b_forward with the chain as the grid's second dimension: two chains that share one
    construction, batched by iterate_many, are each the chain it is alone (and the checker's)."""
    T, K = 1025, 5
    x = ol.trace(T, K, 7)
    alone = [lone_chain(hml, x, K, chain) for chain in range(2)]
    pairs = []
    for chain in range(2):
        o = ol.OracleChain(K=K, seed=9, chain=chain, rng=ol.RNG_CTR, math=ol.MATH_DEV, reduce=ol.REDUCE_DEV, weight_mult=1e9)
        o.load(x)
        g = hml.Chain(device=0, seed=9, chain_id=chain)
        if chain == 0:
            g.load(x)
            g.scale_weights(1e9)   # (before the second chain attaches: shared weights are not rescaled)
        else:
            g.attach(pairs[0][1])
        setup_model(o, g, K)
        o.token("F")
        g.sample_prior()
        o.set_record(marginals=True)
        pairs.append((o, g))
    gs = [g for _, g in pairs]
    for m, n, t in SCHEME:
        for o, _ in pairs:
            o.iterate(m, n, t)
        hml.iterate_many(gs, m, n, t)
    for chain, (o, g) in enumerate(pairs):
        g.sync()
        check(hml, o, g, T, "attached chain %d" % chain)
        A, pi = g.transitions()
        blocks, states, theta, Ab, pib, text = alone[chain]
        assert np.array_equal(blocks, g.blocks()) and np.array_equal(states, g.states()), chain
        assert np.array_equal(theta, bits(g.theta())) and np.array_equal(Ab, bits(A)) and np.array_equal(pib, bits(pi)), chain
        assert text == hml.marginals_text(*g.marginals_rle()), chain
    assert not np.array_equal(gs[0].theta(), gs[1].theta())
    for g in reversed(gs):
        g.close()

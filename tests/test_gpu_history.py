"""The chain's history on the GPU (hml_k_history.h behind hml_set_history / hml_history_read / hml_history_summary).  The
expected rows come from the CPU CHECKER, stepped one sweep per call and evaluated in numpy float64 by tests/history_util.py;
never from the product.  The GPU chain must first equal the checker in blocks, states and theta bits - the history does not
disturb the chain.  Columns 0, 1, 6-10 are compared exactly, columns 2-5 under (addends + 16) 2^-52 sum |addend| (the largest
observed error is printed next to the bound), non-finite entries by kind.  tests/test_history_stats_cpu.py shows on the checker
alone that the rows have something to find and that columns 2 + 3 are the complete-data log-likelihood block by block."""
import gc

import numpy as np
import pytest

from tests import bands_cases as bc
from tests import history_util as hu
from tests import oracle_lib as ol

pytestmark = pytest.mark.gpu


def gpu_chain(hml, c, chain=0, options=(), attach=None, history=True, every=1, seed=None):
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
        g.load(c["trace"]() if callable(c["trace"]) else c["trace"])
    g.set_model(c["K"], g.autoprior(0.2, 0.9))
    if history:
        g.set_history(True, every)
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
        g.iterate(tok[0], tok[1], 0)


def gpu_run(g, scheme):
    for tok in scheme:
        gpu_token(g, tok)
    g.sync()
    return g


def same_chain(g, blocks, states, theta):
    return np.array_equal(blocks, g.blocks()) and np.array_equal(states, g.states()) and np.array_equal(theta.view(np.uint32), g.theta().view(np.uint32))


def run_case(hml, name, c, options=()):
    rows, bounds, blocks, states, theta = hu.expected(name, c)
    g = gpu_run(gpu_chain(hml, c, options=options), c["scheme"])
    assert same_chain(g, blocks, states, theta), name
    got = g.history()
    assert g.history_dropped() == 0
    hu.assert_rows(got, rows, bounds, what=name)
    return g, got, rows


@pytest.mark.parametrize("name", ["k3", "k5", "k10", "k20_wide", "k40_wide", "k4_mixed", "depth", "mv_c22", "compat_k4", "compat_mv"])
def test_history_matches_checker(hml, name):
    """sweep_k (k3, k5; the spread parameter kernel: k10), sweep_wide with M tokens (k20_wide, k40_wide), M, S, P, D and F tokens
    with static blocks and mixture rows (k4_mixed), sums far from unit scale (depth), D = 2 with n_p from the map (mv_c22),
    sweep_compat (compat_k4, compat_mv)"""
    c = bc.CASES[name]
    g, got, rows = run_case(hml, name, c)
    n = sum(t[1] for t in c["scheme"] if not isinstance(t, str))
    assert got.shape == (n, hml.HISTORY_COLS) and np.array_equal(got[:, 0], np.arange(1, n + 1))
    methods = {0.0 if t[0] == "F" else 1.0 for t in c["scheme"] if not isinstance(t, str)}
    assert set(got[:, 1]) == methods
    assert [hml.history_column(i) for i in range(12)] == list(hu.COLS) + [None] and tuple(hml.HISTORY_COLUMNS) == hu.COLS
    g.close()


def test_history_weakly_compressed(hml, monkeypatch):
    """k5 with the geometry of weakly compressed sweeps forced on from the first block (the fused trellis kernels)"""
    monkeypatch.setenv("HML_DENSE_MIN_BLOCKS", "1")
    g, got, rows = run_case(hml, "k5", bc.CASES["k5"])
    g.close()


def test_history_iterate_many_equals_iterate_bit_for_bit(hml):
    """three chains attached to one trace through hml_iterate_many, history on for chains 0 and 2 only: each history is that of
    the same chain run alone through hml_iterate, bit for bit - and the checker's; chain 1 has no buffer: after a first batched
    sweep (which makes the batch's own allocations) the library allocates two buffers more, not three"""
    c = dict(bc.CASES["k5"], seed=21, scheme=[("F", 12, 0), ("F", 18, 0)])
    alone = {}
    for k in (0, 2):
        g = gpu_chain(hml, c, chain=k, history=False)
        gpu_token(g, ("F", 1, 0))
        g.set_history(True)
        alone[k] = gpu_run(g, c["scheme"]).history()
        g.close()
    gc.collect()
    live0 = hml.device_memory_live()
    first = gpu_chain(hml, c, chain=0, history=False)
    chains = [first] + [gpu_chain(hml, c, chain=k, attach=first, history=False) for k in (1, 2)]
    for g in chains:
        g.sample_prior()
        g._pending_prior = False
    hml.iterate_many(chains, "F", 1, 0)
    for g in chains:
        g.sync()
    allocations = hml.device_memory_live()[1]
    chains[0].set_history(True)
    chains[2].set_history(True)
    for m, n, t in c["scheme"]:
        hml.iterate_many(chains, m, n, t)
    for g in chains:
        g.sync()
    assert hml.device_memory_live()[1] == allocations + 2
    assert chains[1].history().shape == (0, 11) and chains[1].history_dropped() == 0
    for k in (0, 2):
        got = chains[k].history()
        assert got.shape == (30, 11) and hu.same_bits(got, alone[k]), k
        assert np.all(got[:, 10] == k) and np.array_equal(got[:, 0], np.arange(2, 32))
        o, prior = hu.checker(c, chain=k)
        rows, bounds = hu.walk(o, prior, [("F", 1, 0)] + c["scheme"], chain=k)
        assert same_chain(chains[k], o.blocks(), o.states(), o.theta())
        o.close()
        hu.assert_rows(got, rows[1:], bounds[1:], what="iterate_many chain %d" % k)
    for g in chains:
        g.close()
    assert hml.device_memory_live() == live0


def test_history_of_a_halted_chain(hml):
    """max_blocks = 64 on k5: the chain halts and settles (hml_settle runs the skipped sweeps again); the history has the same
    rows, bit for bit, as the unrestricted chain - none missing, none twice"""
    c = bc.CASES["k5"]
    g0 = gpu_run(gpu_chain(hml, c, every=2), c["scheme"])
    g1 = gpu_run(gpu_chain(hml, c, every=2, options=(("max_blocks", 64),)), c["scheme"])
    assert g0.stats()["buffer_growths"] == 0 and g1.stats()["buffer_growths"] > 0
    ref, got = g0.history(), g1.history()
    n = sum(t[1] for t in c["scheme"])
    assert ref.shape == (n // 2, 11) and hu.same_bits(ref, got)
    assert np.array_equal(got[:, 0], 2.0 * np.arange(1, n // 2 + 1)) and g1.history_dropped() == 0
    rows, bounds, blocks, states, theta = hu.expected("k5", c)      # (every sweep's row: the even sweeps of it)
    assert same_chain(g1, blocks, states, theta)
    hu.assert_rows(got, rows[1::2], bounds[1::2], what="max_blocks 64")
    g0.close()
    g1.close()


def test_history_thinning_and_growth(hml):
    """every = 3 over four iterate calls of 1, 2, 50 and 500 sweeps on 20 000 positions: the rows are exactly the sweeps divisible
    by 3, the buffer grew at least twice (the device memory the library holds rose in two of the calls), nothing was dropped;
    off and on keeps the rows; clear_history empties it"""
    c = dict(bc.CASES["k3"], T=20000, trace=lambda: ol.trace(20000, 3, 7), seed=9)
    g = gpu_chain(hml, c, every=3)
    g.sample_prior()
    held, total = [], 0
    for n in (1, 2, 50, 500):
        g.iterate("F", n, 0)
        g.sync()
        total += n
        held.append(hml.device_memory_live()[0])
        assert np.array_equal(g.history()[:, 0], np.arange(3, total + 1, 3)), n
    assert sum(b > a for a, b in zip(held, held[1:])) >= 2, held
    assert g.history_dropped() == 0
    kept = g.history()
    g.set_history(False)
    g.iterate("F", 6, 0)
    g.set_history(True, 3)
    g.iterate("F", 6, 0)
    g.sync()
    got = g.history()
    assert hu.same_bits(got[: len(kept)], kept) and np.array_equal(got[len(kept):, 0], [561.0, 564.0])
    # the first rows against the checker (the 553 sweeps are not stepped on the CPU: 60 of them)
    o, prior = hu.checker(c)
    rows, bounds = hu.walk(o, prior, [("F", 60, 0)], every=3)
    o.close()
    hu.assert_rows(got[:20], rows, bounds, what="every 3")
    g.clear_history()
    assert g.history().shape == (0, 11) and g.history_dropped() == 0
    g.iterate("F", 3, 0)
    assert np.array_equal(g.history()[:, 0], [567.0])
    with pytest.raises(hml.HmlError) as e:
        g.set_history(True, 0)
    assert e.value.code == 1 and "at least 1" in str(e.value)
    g.close()


def test_history_under_graph_replay(hml, monkeypatch):
    """HML_USE_GRAPH=1: a captured sweep contains the history launch - the same bits as the eager run; turning the history on
    after a sweep was captured drops the graph"""
    c = dict(bc.CASES["k3"], scheme=[("F", 40, 0)])
    eager = gpu_run(gpu_chain(hml, c), c["scheme"])
    want, th = eager.history(), eager.theta()
    eager.close()
    monkeypatch.setenv("HML_USE_GRAPH", "1")
    g = gpu_run(gpu_chain(hml, c), c["scheme"])
    assert hu.same_bits(g.history(), want) and np.array_equal(g.theta().view(np.uint32), th.view(np.uint32))
    g.close()
    late = gpu_chain(hml, c, history=False)
    late.sample_prior()
    late._pending_prior = False
    late.iterate("F", 10, 0)                 # captured without the launch
    late.set_history(True, 1)
    late.iterate("F", 30, 0)
    late.sync()
    assert hu.same_bits(late.history(), want[10:])
    late.close()


FAMILIES = ["blocks_compact", "blocks_scatter", "stats_emission", "emission", "trellis", "trellis_repair", "forward", "backward_maps",
            "backward_chain", "mixture", "counts", "marginals", "params", "levels", "breaks", "bands", "regions", "history"]


def test_history_off_means_off(hml):
    """history never turned on: the launches per family over 20 sweeps are those of today's sweep (the counts of
    tests/test_gpu_sweep_paths.py's default case) and none of the family "history"; with it on, one per sweep and the chain's
    bits are the same"""
    gc.collect()
    c = dict(bc.CASES["k3"], T=200000, trace=lambda: ol.trace(200000, 3, 8), seed=3, scheme=[("F", 20, 0)])
    N = 20
    kept = []
    for on in (False, True):
        g = gpu_chain(hml, c, history=on)
        g.sample_prior()
        g.profile_enable(2)
        g.iterate("F", N, 0)
        g.sync()
        g.profile_enable(0)
        counts = {f: g.profile_get(f)[1] for f in FAMILIES}
        want = dict(blocks_compact=N + 1, blocks_scatter=1, forward=N, backward_maps=N, backward_chain=N, counts=N, params=N, history=N if on else 0)
        assert counts == {f: want.get(f, 0) for f in FAMILIES}, on
        assert g.history().shape == ((N if on else 0), 11)
        kept.append((g.blocks(), g.states(), g.theta().view(np.uint32)))
        g.close()
    assert all(np.array_equal(a, b) for a, b in zip(*kept))


def test_history_memory_goes_with_the_context(hml):
    gc.collect()
    live0 = hml.device_memory_live()
    c = dict(bc.CASES["k3"], T=20000, trace=lambda: ol.trace(20000, 3, 7), seed=9)
    g = gpu_chain(hml, c)
    g.sample_prior()
    for n in (5, 40, 300):
        g.iterate("F", n, 0)
    assert g.history().shape == (345, 11)
    g.close()
    assert hml.device_memory_live() == live0


def test_history_summary(hml):
    """history_summary over four chains of k3 with different chain_ids = history_stats of the rows read back, bit for bit, and
    R-hat and ESS equal the numpy restatement within 1e-10 relative: double arithmetic in another order - sums of h = 7 terms
    (rounding 7 2^-53 of sum |term|) in W, B and seven autocovariances, a few hundred operations in all"""
    c = bc.CASES["k3"]                       # 30 sweeps
    chains = [gpu_run(gpu_chain(hml, c, chain=k), c["scheme"]) for k in range(4)]
    hist = [g.history() for g in chains]
    for col, pick in (("loglik", lambda h: h[:, 2] + h[:, 3]), ("logpost", lambda h: ((h[:, 2] + h[:, 3]) + h[:, 4]) + h[:, 5]),
                      ("segments", lambda h: h[:, 6]), (7, lambda h: h[:, 7])):
        x = np.stack([pick(h)[-14:] for h in hist])          # sweeps 17 ... 30
        s = hml.history_summary(chains, col, skip_sweeps=16)
        t = hml.history_stats(x)
        want = hu.stats(x)
        print(col, "rhat %.6g ess %.6g" % (s["rhat"], s["ess"]))
        assert s["n_used"] == 14 and s["n_nonfinite"] == t["n_nonfinite"] == want["n_nonfinite"]
        for k in ("rhat", "ess", "chain_mean", "chain_sd"):
            a, b, w = np.atleast_1d(s[k]), np.atleast_1d(t[k]), np.atleast_1d(want[k])
            assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), (col, k)
            assert np.array_equal(np.isnan(a), np.isnan(w)) and np.allclose(a[~np.isnan(a)], w[~np.isnan(w)], rtol=1e-10, atol=0), (col, k, a, w)
    # the rows of the shortest chain decide how many are used
    chains[1].iterate("F", 4, 0)
    assert hml.history_summary(chains, "loglik", skip_sweeps=0)["n_used"] == 30
    with pytest.raises(hml.HmlError) as e:
        hml.history_summary(chains, "loglik", skip_sweeps=25)           # h = 2
    assert e.value.code == 1 and "at least 8 values" in str(e.value)
    with pytest.raises(hml.HmlError):
        hml.history_summary(chains, 11)
    for g in chains:
        g.close()

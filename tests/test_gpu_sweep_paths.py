"""Which path a sweep takes - on the default path, in the reference-compatible mode and beyond 16 states - seen through the
per-family launch counters (profile level 2: every family bracketed, one count per bracket).  The plan of a sweep
(hammlet_amd/csrc/hml_sweep_plan.h, hml_rtk_plan.h) never changes its results, so each case also runs the same chain with
profiling off and compares states and theta bit for bit.

The expected counts are those of the commit before each plan existed (its library ran this file).  The counters cannot tell the
mid geometry from the sparse one (same kernels, another chunk length), the scan variants of the scan + scatter pair from
each other (one family), nor one chunk from many or a chunk a lane from a state a lane: tests/test_sweep_plan_cpu.py and
tests/test_rtk_plan_cpu.py hold those."""
import gc

import numpy as np
import pytest

from tests import oracle_lib as ol

pytestmark = pytest.mark.gpu

N = 12   # sweeps per case
FAMILIES = ["blocks_compact", "blocks_scatter", "stats_emission", "emission", "trellis", "trellis_repair", "forward", "backward_maps",
            "backward_chain", "mixture", "counts", "marginals", "params"]

DENSE = {"HML_DENSE_MIN_BLOCKS": "1"}
# per case: how the chain is set up, and the launches of every family over N sweeps.  One enumeration ahead of the first sweep
# (the hint predates the prior draw) adds a scan + scatter pair: blocks_compact N + 1 where every sweep has a block launch.
CASES = {
    # the fused block kernel makes starts, statistics and emission terms: no scatter but the enumeration's
    "default": (dict(), dict(blocks_compact=N + 1, blocks_scatter=1, forward=N, backward_maps=N, backward_chain=N, counts=N, params=N)),
    "fused_blocks_0": (dict(options=[("fused_blocks", 0)]),
                       dict(blocks_compact=N + 1, blocks_scatter=N + 1, stats_emission=N, forward=N, backward_maps=N, backward_chain=N, counts=N, params=N)),
    "second_context": (dict(other=True),
                       dict(blocks_compact=N + 1, blocks_scatter=N + 1, stats_emission=N, forward=N, backward_maps=N, backward_chain=N, counts=N, params=N)),
    # many blocks: the fused trellis kernels make the emission terms themselves
    "dense": (dict(env=DENSE), dict(blocks_compact=N + 1, blocks_scatter=1, trellis=N, trellis_repair=N, backward_chain=N, counts=N, params=N)),
    "dense_separate": (dict(env=dict(DENSE, HML_TRELLIS_FUSED="0")),
                       dict(blocks_compact=N + 1, blocks_scatter=1, forward=N, backward_maps=N, backward_chain=N, counts=N, params=N)),
    "dense_tile": (dict(env=dict(DENSE, HML_TRELLIS_ROWS="0")),
                   dict(blocks_compact=N + 1, blocks_scatter=1, trellis=N, trellis_repair=N, backward_chain=N, counts=N, params=N)),
    "mid": (dict(env={"HML_MID_MIN_BLOCKS": "200"}),
            dict(blocks_compact=N + 1, blocks_scatter=1, forward=N, backward_maps=N, backward_chain=N, counts=N, params=N)),
    "mixture": (dict(method="M"), dict(blocks_compact=N + 1, blocks_scatter=1, mixture=N, counts=N, params=N)),
    # static blocks: the first sweep enumerates, the others compute emission terms only
    "static": (dict(static=True), dict(blocks_compact=2, blocks_scatter=1, emission=N - 1, forward=N, backward_maps=N, backward_chain=N, counts=N, params=N)),
    "two_dims": (dict(dims=(2, 2), K=4),
                 dict(blocks_compact=N + 1, blocks_scatter=N + 1, stats_emission=N, forward=N, backward_maps=N, backward_chain=N, counts=N, params=N)),
    # every position a block: the float stream (flag staging / the plain scan), never the fused kernel
    "every_position": (dict(scale=1e9),
                       dict(blocks_compact=N + 1, blocks_scatter=N + 1, stats_emission=N, forward=N, backward_maps=N, backward_chain=N, counts=N, params=N)),
    "every_position_plain_scan": (dict(scale=1e9, env={"HML_STAGE_BITS": "0"}),
                                  dict(blocks_compact=N + 1, blocks_scatter=N + 1, stats_emission=N, forward=N, backward_maps=N, backward_chain=N, counts=N, params=N)),
    # The two paths that take the number of states at run time (hml_rtk_sweep.hpp; their plan: tests/test_rtk_plan_cpu.py).  Every
    # sweep enumerates with the scan + scatter pair and nothing runs ahead of the first.  The reference-compatible mode brackets its
    # filter and its backward draws only - the marginals of a recorded sweep too go unbracketed there - the path for more than
    # 16 states also emission terms, count tree and parameter kernel.  A chunk a lane or a state a lane, one chunk or seven: the
    # same two brackets.
    "compat": (dict(options=[("compat", 1)]), dict(blocks_compact=N, blocks_scatter=N, forward=N, backward_maps=N)),
    "compat_chunks_7": (dict(options=[("compat", 1)], env={"HML_COMPAT_CHUNKS": "7"}), dict(blocks_compact=N, blocks_scatter=N, forward=N, backward_maps=N)),
    "compat_mixture": (dict(options=[("compat", 1)], method="M"), dict(blocks_compact=N, blocks_scatter=N)),
    "compat_recorded": (dict(options=[("compat", 1)], thinning=3), dict(blocks_compact=N, blocks_scatter=N, forward=N, backward_maps=N)),
    "wide_k3": (dict(env={"HML_WIDE": "1"}), dict(blocks_compact=N, blocks_scatter=N, stats_emission=N, forward=N, backward_maps=N, counts=N, params=N)),
    "wide_k20": (dict(K=20), dict(blocks_compact=N, blocks_scatter=N, stats_emission=N, forward=N, backward_maps=N, counts=N, params=N)),
    "wide_state_a_lane": (dict(K=20, env={"HML_WIDE_LANES": "0"}),
                          dict(blocks_compact=N, blocks_scatter=N, stats_emission=N, forward=N, backward_maps=N, counts=N, params=N)),
    "wide_mixture": (dict(K=20, method="M"), dict(blocks_compact=N, blocks_scatter=N, stats_emission=N, counts=N, params=N)),
}

# The trace: 200 000 positions in about 830 blocks at K = 3 (1440 with two dimensions), a hint of about 2060 (2830).  The
# fused block kernel runs while hint * 24 <= T, that is up to a hint of 8333 or some 5800 blocks: seven times what the
# trace has ("default", "dense", "mid", ...: blocks_scatter = 1).  With every position a block the hint is 251 024, thirty
# times beyond it.  Each case prints its block count.
T = 200_000
_traces = {}


def trace(dims):
    if dims not in _traces:
        x = ol.trace(T, 3, 8)
        _traces[dims] = x if dims is None else np.stack([x, ol.trace(T, 3, 9)], axis=1).reshape(-1)
    return _traces[dims]


def run(hml, setup, profile):
    """the chain of a case over N sweeps: (launches per family, states, theta, blocks of the last sweep)"""
    K = setup.get("K", 3)
    g = hml.Chain(device=0, seed=3)
    other = hml.Chain(device=0, seed=4) if setup.get("other") else None   # a second live context on the same device
    try:
        for name, value in setup.get("options", ()):
            g.set_option(name, value)
        if setup.get("dims"):
            g.set_dimensions(*setup["dims"])
        g.load(trace(setup.get("dims")))
        if setup.get("scale"):
            g.scale_weights(setup["scale"])
        g.set_model(K, g.autoprior(0.2, 0.9))
        g.sample_prior()
        if setup.get("static"):
            g.set_dynamic(0)
        g.profile_enable(2 if profile else 0)
        before = {f: g.profile_get(f)[1] for f in FAMILIES}
        g.iterate(setup.get("method", "F"), N, setup.get("thinning", 0))
        g.sync()
        g.profile_enable(0)
        counts = {f: g.profile_get(f)[1] - before[f] for f in FAMILIES}
        return counts, g.states().copy(), g.theta().copy(), g.num_blocks()
    finally:
        if other is not None:
            other.close()
        g.close()


@pytest.mark.parametrize("case", list(CASES))
def test_sweep_takes_the_planned_path(hml, monkeypatch, case):
    gc.collect()   # (no context of an earlier test left alive on the device: it would count as a second one)
    setup, want = CASES[case]
    for name, value in setup.get("env", {}).items():
        monkeypatch.setenv(name, value)
    counts, q, th, blocks = run(hml, setup, profile=True)
    print(case, "blocks", blocks, {f: n for f, n in counts.items() if n})
    assert counts == {f: want.get(f, 0) for f in FAMILIES}
    _, q0, th0, _ = run(hml, setup, profile=False)
    assert np.array_equal(q, q0) and np.array_equal(th.view(np.uint32), th0.view(np.uint32))


# The carved buffers of the two run-time-K paths (hml_layouts.h) are laid out again at every growth of the block capacity.
T_GROWTH = 20_000
GROWTH = {"compat": (3, [("compat", 1)]), "wide_k20": (20, [])}


def grown_chain(hml, x, K, options, max_blocks):
    g = hml.Chain(device=0, seed=5)
    try:
        for name, value in options:
            g.set_option(name, value)
        if max_blocks:
            g.set_option("max_blocks", max_blocks)
        g.load(x)
        g.set_model(K, g.autoprior(0.2, 0.9))
        g.sample_prior()
        g.iterate("F", N, 0)
        g.sync()
        A, pi = g.transitions()
        return g.states().copy(), g.theta().copy(), np.array(A).copy(), np.array(pi).copy(), g.stats()
    finally:
        g.close()


@pytest.mark.parametrize("case", list(GROWTH))
def test_a_chain_that_grows_is_the_chain_at_full_capacity(hml, case):
    K, options = GROWTH[case]
    x = ol.trace(T_GROWTH, 3, 8)
    q, th, A, pi, st = grown_chain(hml, x, K, options, 64)
    q0, th0, A0, pi0, st0 = grown_chain(hml, x, K, options, 0)
    print(case, "growths", st["buffer_growths"], "capacity", st["block_capacity"], "blocks", len(q))
    assert st["buffer_growths"] >= 1 and st["block_capacity"] > 64 and st0["buffer_growths"] == 0
    assert np.array_equal(q, q0)
    for a, b in ((th, th0), (A, A0), (pi, pi0)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))

"""The contexts own their device memory (DevBuf / DevArr, hml_host_common.hpp): whatever a chain allocated goes with it, an
allocation that fails leaves a context that can be closed or asked again, and a growth of the per-block buffers that fails
changes no chain.  hml_device_memory_live counts what the owners hold; hml_debug_fail_allocation makes the n-th allocation
fail, which is the only way to reach these paths on demand.

The cases that only create, run and destroy come first; the ones that go on with a context after a failed call follow.  After
a HIP error that is not the injected one a test does nothing more with that context but close it."""
import gc

import numpy as np
import pytest

from tests import oracle_lib as ol
from tests.test_gpu_parity import bits, compare_state

pytestmark = pytest.mark.gpu

HML_ERR_HIP = 2
T = 4096


def live(hml, collect=False):
    """(bytes, allocations) the owners hold; collect: chains that earlier tests dropped without closing go first"""
    if collect:
        gc.collect()
    return hml.device_memory_live()


@pytest.fixture(scope="module")
def x3():
    return ol.trace(T, 3, 1)


@pytest.fixture(scope="module")
def x_growth():
    return ol.trace(20000, 5, 12)


def injected(e):
    """the failure the hook made: HML_ERR_HIP from an owner's alloc"""
    return e.code == HML_ERR_HIP and "alloc(" in str(e) and "out of memory" in str(e)


# ------------------------------------------------------------------------------------------------ nothing is left behind
def _plain(hml, x, K=3, options=(), dims=None, probes=False, recordings=False):
    g = hml.Chain(device=0, seed=3)
    for name, value in options:
        g.set_option(name, value)
    if dims:
        g.set_dimensions(*dims)
    g.load(x)
    g.set_model(K, g.autoprior())
    if probes:
        g.enable_probes(True)
    if recordings:
        g.set_level_recording(True)
        g.set_break_recording(True)
        g.set_level_bands([-0.5, 0.5])
        g.set_regions([0, 100, 4000], [50, 300, 4096], edges=[0.0])
    g.iterate("F", 5, 5)   # a handful of sweeps, the last one recorded
    g.sync()
    seg, cnt = g.marginals_rle()
    assert int(seg.sum()) == g.T
    if probes:
        assert g.forward_rows().shape[1] == K
    if recordings:
        g.levels_rle()
        g.breaks_list()
        g.bands_rle()
        g.regions()
    return [g]


def _attached(hml, x):
    src = hml.Chain(device=0, seed=3)
    src.load(x)
    gs = []
    for chain in range(3):
        g = hml.Chain(device=0, seed=3, chain_id=chain + 1)
        g.attach(src)
        g.set_model(3, g.autoprior())
        gs.append(g)
    hml.iterate_many(gs, "F", 5, 5)
    for g in gs:
        g.sync()
    return [src] + gs   # (closed in this order: the source first)


def _growth(hml, x):
    g = hml.Chain(device=0, seed=9)
    g.set_option("max_blocks", 64)
    g.load(x)
    g.set_model(5, g.autoprior())
    g.sample_prior()
    g.iterate("F", 5, 5)
    g.sync()
    st = g.stats()
    assert st["buffer_growths"] >= 1 and st["block_capacity"] > 64, st
    return [g]


def _no_model(hml, x):
    g = hml.Chain(device=0, seed=3)
    g.load(x)
    return [g]


CASES = {
    "default_k3": (lambda hml, x, xg: _plain(hml, x), {}),
    "compat": (lambda hml, x, xg: _plain(hml, x, options=[("compat", 1)]), {}),
    "k20": (lambda hml, x, xg: _plain(hml, x, K=20), {}),
    "d2_p2": (lambda hml, x, xg: _plain(hml, np.stack([x, ol.trace(T, 3, 2)], axis=1).reshape(-1), K=4, dims=(2, 2)), {}),
    "probes": (lambda hml, x, xg: _plain(hml, x, probes=True), {}),
    "recordings": (lambda hml, x, xg: _plain(hml, x, recordings=True), {}),
    "trellis_buffers": (lambda hml, x, xg: _plain(hml, x), {"HML_DENSE_MIN_BLOCKS": "1"}),
    "attached_many": (lambda hml, x, xg: _attached(hml, x), {}),
    "max_blocks_64": (lambda hml, x, xg: _growth(hml, xg), {}),
    "fused_debug": (lambda hml, x, xg: _plain(hml, x), {"HML_FUSED_DEBUG": "1"}),   # (its stamp buffer was in no free list)
    "no_model": (lambda hml, x, xg: _no_model(hml, x), {}),
}


@pytest.mark.parametrize("case", list(CASES))
def test_a_closed_chain_leaves_nothing_behind(hml, monkeypatch, x3, x_growth, case):
    """The live totals (bytes, allocations) after every chain of the case is closed are the totals from before it."""
    run, env = CASES[case]
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    before = live(hml, collect=True)
    chains = run(hml, x3, x_growth)
    held = live(hml)
    assert held[0] > before[0] and held[1] > before[1], (before, held)
    for g in chains:
        g.close()
    assert live(hml) == before


# ------------------------------------------------------------------ a failed allocation: nothing left behind, and once more
PATHS = {"default": (3, []), "compat": (3, [("compat", 1)]), "k20": (20, [])}
_checkers = {}


def checker(path, x):
    """the checker's chain of the path after 4 FB sweeps (computed once; the tests only read it)"""
    if path not in _checkers:
        K = PATHS[path][0]
        if path == "compat":
            o = ol.OracleChain(K=K, seed=3, rng=ol.RNG_MT, math=ol.MATH_LIBM, reduce=ol.REDUCE_REF)
        else:
            o = ol.OracleChain(K=K, seed=3, rng=ol.RNG_CTR, math=ol.MATH_DEV, reduce=ol.REDUCE_DEV)
        o.load(x)
        prior = o.autoprior()
        o.init_model()
        o.token("F")
        o.iterate("F", 4, 0)
        _checkers[path] = (o, prior)
    return _checkers[path]


def _fresh(hml, path, call, x):
    """(chain, the call under test, chains to close besides it)"""
    K, options = PATHS[path]
    g = hml.Chain(device=0, seed=3)
    for name, value in options:
        g.set_option(name, value)
    if call == "load":
        return g, (lambda: g.load(x)), []
    if call == "attach":
        src = hml.Chain(device=0, seed=3, chain_id=7)
        for name, value in options:
            src.set_option(name, value)
        src.load(x)
        return g, (lambda: g.attach(src)), [src]
    g.load(x)
    prior = g.autoprior()
    return g, (lambda: g.set_model(K, prior)), []


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("call", ["load", "attach", "set_model"])
def test_a_failed_allocation_leaves_nothing_behind_and_the_call_can_be_made_again(hml, x3, call, path):
    """Every allocation of the call fails in turn, on a fresh chain each: HML_ERR_HIP; the context holds no more than the
    buffers allocated before the one that failed (the call's scratch is gone); the same call made again succeeds, leaves
    exactly what a call that never failed leaves, and the chain is the checker's after 4 FB sweeps, bit for bit; closing
    returns everything.  The first n the call does not reach ends the walk: n - 1 allocations is what the call makes."""
    K = PATHS[path][0]
    o, prior_o = checker(path, x3)
    baseline = live(hml, collect=True)
    retried, clean = [], None
    for n in range(1, 64):
        g, fn, others = _fresh(hml, path, call, x3)
        before = live(hml)
        hml.debug_fail_allocation(n)
        try:
            fn()
            failure = None
        except hml.HmlError as e:
            failure = e
        finally:
            made = hml.debug_fail_allocation(0)
        if failure is not None and not injected(failure):
            for c in [g] + others:
                c.close()
            raise failure
        if failure is None:
            assert made == n - 1, (made, n)   # the hook was never reached
            clean = tuple(a - b for a, b in zip(live(hml), before))
        else:
            assert made == n, (made, n)
            after = live(hml)
            assert before[1] <= after[1] <= before[1] + n - 1 and after[0] >= before[0], (n, before, after)
            if after[1] == before[1]:
                assert after[0] == before[0]
            fn()   # once more, on the same chain
            retried.append(tuple(a - b for a, b in zip(live(hml), before)))
            if call != "set_model":
                prior = g.autoprior()
                if path != "compat":
                    assert np.array_equal(bits(prior), bits(prior_o))
                g.set_model(K, prior)
            g.sample_prior()
            g.iterate("F", 4, 0)
            g.sync()
            compare_state(o, g, what="%s %s, allocation %d failed once" % (path, call, n))
        for c in [g] + others:
            c.close()
        assert live(hml) == baseline, n
        if failure is None:
            break
    assert clean is not None, "the call still reached the hook at n = 63"
    assert retried and all(r == clean for r in retried), (clean, retried)
    print("allocations of %s on path %s: %d" % (call, path, n - 1))


# ------------------------------------------------------------------------------------------- a failed growth changes no chain
def test_a_failed_growth_changes_no_chain(hml, x_growth):
    """Per-block buffers for 512 blocks; the checker's FB sweeps need 355, 340, 952, ... blocks: the first two sweeps of the call
    run, the third halts the chain, and the growth is made while the model's sweep counter is two ahead of the log's base -
    where hml_settle's bookkeeping has to survive a growth that fails.  Every allocation of the growth fails in turn, on a
    fresh chain each: HML_ERR_HIP; then the chain settles, finishes the call's sweeps and is the checker's chain bit for bit,
    marginals included, every recorded sweep called back exactly once, 8 sweeps counted.

    With a callback on every second sweep hml_iterate waits for sweep 3 and finds the chain halted, so the growth - and the
    error - is hml_iterate's own, not the following hml_sync's: the hook is set from the callback of sweep 1, the last moment
    before the growth (the marginals' buffers exist by then), the failed call's remaining sweeps are asked for again one by
    one, and the callbacks are compared by the sweep's place in the eight."""
    K = 5
    o = ol.OracleChain(K=K, seed=9, chain=0, rng=ol.RNG_CTR, math=ol.MATH_DEV, reduce=ol.REDUCE_DEV)
    o.load(x_growth)
    prior = o.autoprior()
    o.init_model()
    o.token("F")
    o.set_record(marginals=True)
    blocks = []
    for i in range(8):
        o.iterate("F", 1, 1 if i % 2 else 0)
        blocks.append(int(o.num_blocks()))
    print("checker's blocks per sweep:", blocks)
    assert max(blocks[:2]) <= 512 < max(blocks[2:]), blocks
    want = o.text("marginals")
    baseline = live(hml, collect=True)

    def run(n):
        """a fresh chain whose n-th allocation from sweep 1's callback on fails; returns (allocations made, failure)"""
        g = hml.Chain(device=0, seed=9, chain_id=0)
        g.set_option("max_blocks", 512)
        g.load(x_growth)
        pg = g.autoprior(0.2, 0.9)
        assert np.array_equal(bits(prior), bits(pg))
        g.set_model(K, pg)
        g.sample_prior()
        seen, first = [], [0]

        def callback(ch, sweep):
            seen.append(first[0] + int(sweep))
            if first[0] == 0 and sweep == 1:
                hml.debug_fail_allocation(n)

        g.set_recording(marginals=True, callback=callback)
        st = g.stats()
        assert st["buffer_growths"] == 0 and st["block_capacity"] == 512, st
        try:
            try:
                g.iterate("F", 8, 2)
                failure = None
            except hml.HmlError as e:
                failure = e
            finally:
                made = hml.debug_fail_allocation(0)
            if failure is not None:
                if not injected(failure):
                    raise failure
                g.sync()   # grows, and runs again what the halted chain skipped
                done = int(g.stats()["sweeps"])
                assert 3 <= done <= 4, done   # (the call stopped at its sweep 3, before or after enqueueing it)
                for i in range(done, 8):
                    first[0] = i
                    g.iterate("F", 1, 1 if i % 2 else 0)
            g.sync()
            what = "allocation %d of the growth failed once" % n
            compare_state(o, g, what=what)
            seg, cnt = g.marginals_rle()
            assert hml.marginals_text(seg, cnt) == want, what
            assert seen == [1, 3, 5, 7], (what, seen)
            st = g.stats()
            assert st["sweeps"] == 8 and st["buffer_growths"] >= 1, (what, st)
        finally:
            g.close()
        assert live(hml) == baseline, n
        return made, failure, int(st["buffer_growths"])

    N, failure, growths = run(1 << 40)   # (never reached: the allocations one growth makes)
    assert failure is None and 2 <= N < 64, (N, failure)
    print("allocations of a growth:", N)
    for n in range(1, N + 1):
        made, failure, grown = run(n)
        assert failure is not None and made == n and grown == growths, (n, made, failure, grown)

"""The count read-outs of the smoothing on the device (hml_posterior_region_counts, hml_posterior_count_terms,
hml_posterior_counts_info, include/hml.h) against the restatement for one host thread, tests/fixtures/counts_ref_main.cpp over
hammlet_amd/csrc/hml_counts_ref.h, which is fed the GPU's own block_stats(), blocks(), theta() and transitions().  Every double
- v, rho, the histograms, whole_state, avoid - is compared as its 64-bit word: there is no tolerance in the word comparisons of
this file.

The later sections compare with the other read-outs, each within a bound that is derived and not measured: with
hml_posterior_regions within twice the quantisation bound include/hml.h derives for it; with the sample of
hml_posterior_sample_regions within Bernstein's bound at delta = 1e-12 per cell (tests/sample_util.bernstein)."""
import gc

import numpy as np
import pytest

from tests import counts_util as cu
from tests import hostile_inputs as hi
from tests import infer_cases as ic
from tests import oracle_lib as ol
from tests import pairs_util as pz
from tests import posterior_util as pu
from tests import sample_util as su
from tests.infer_fuzz_util import NIG4
from tests.test_gpu_pairs import chain

pytestmark = pytest.mark.gpu

GRID = 4096                # regions a grid of the walks takes at once (a workgroup a region)
SLICE = 16                 # struck-out states a workgroup of the avoidance walk holds
N_RANDOM = 2000


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return cu.build_programs(tmp_path_factory.mktemp("counts_ref"), sanitized=False)["plain"]


def regions_of(g, n_random, every_length=False):
    starts = g.blocks()
    rng = np.random.default_rng(g.num_blocks())
    start, end = pz.edge_regions(starts, rng, n_random)
    if every_length:       # be - ba = 0 ... B - 1, from the first block
        start = np.concatenate([start, np.zeros(len(starts) - 1, np.uint32)])
        end = np.concatenate([end, np.asarray(starts[1:], np.uint32)])
    return start, end


def check(hml, program, g, H=8, self_trans=True, what=None, n_random=N_RANDOM, every_length=False, regions=None):
    """the terms, the regions' words and the numbers about the call equal the restatement's"""
    case = pu.chain_case(g, self_trans)
    start, end = regions or regions_of(g, n_random, every_length)
    want = cu.run_program(program, case, start, end, H)
    t = g.posterior_count_terms()
    for key in ("v", "rho"):
        assert np.array_equal(pu.words(t[key]), want[key].ravel()), (what, key)
    r = g.posterior_region_counts(start, end, H)
    assert r["count_degenerate"] == want["count_degenerate"], what
    assert r["hist"].shape == (len(start), H + 1) and r["whole_state"].shape == r["avoid"].shape == (len(start), g.K)
    cu.same_regions(cu.region_words(r), want, what)
    for key in cu.REGION_KEYS:
        assert not np.isnan(r[key]).any(), (what, key)
    assert g.posterior_counts_info() == dict(regions=len(start), steps=want["steps"], longest=want["longest"]), what
    return want, r, (start, end)


def steps_of(g, start, end):
    starts = np.asarray(g.blocks(), np.int64)
    block = lambda p: np.searchsorted(starts[:-1], np.asarray(p, np.int64), side="right") - 1
    return block(np.asarray(end, np.int64) - 1) - block(start)


# ---------------------------------------------------------------------------------------------- shapes
@pytest.mark.parametrize("T", [2, 3, 16, 65])
def test_tiny_traces(hml, program, T):
    g = chain(hml, ol.trace(1000, 3, 2)[:T].copy(), 2, seed=12, sweeps=10)
    want, _, _ = check(hml, program, g, what=T, n_random=50)
    assert want["count_degenerate"] == 0


def test_one_block(hml, program):
    """no step: hist = [1, 0, ...] and avoid[j] = 1 - gamma_0(j)"""
    g = hml.Chain(device=0, seed=12)
    g.load(np.array([0.3], np.float32))
    g.set_model(2, np.array([2.0, 1.0, 0.0, 1.0], np.float32))
    g.sample_prior()
    g.create_blocks(1.0)
    assert g.num_blocks() == 1
    _, r, _ = check(hml, program, g, what="B = 1", n_random=0)
    gamma = g.posterior()[0]
    assert np.all(np.abs(r["hist"][:, 0] - 1.0) <= 1e-15) and not r["hist"][:, 1:].any()
    assert np.all(np.abs(r["avoid"] - (1.0 - gamma[0])) <= 1e-15)
    assert np.array_equal(pu.words(r["whole_state"][0]), pu.words(gamma[0]))
    assert g.posterior_counts_info()["steps"] == 0


def test_every_position_a_block_and_every_length(hml, program):
    """B = 300: regions with be - ba = 0, 1, ... 299"""
    B = 300
    g = chain(hml, ol.trace(B, 5, 4), 5, every_position=True)
    assert g.num_blocks() == B
    want, r, (start, end) = check(hml, program, g, what=B, every_length=True)
    assert want["count_degenerate"] == 0 and want["longest"] == B - 1
    assert set(steps_of(g, start, end).tolist()) >= set(range(B))
    n = steps_of(g, start, end)
    assert np.all(np.abs(r["hist"].sum(axis=1) - 1.0) <= (n + 1) * g.K * 2.0 ** -50)


@pytest.mark.parametrize("K", [2, 3, 5, 8, 9, 16, 17, 32, 33, 64])
def test_numbers_of_states(hml, program, K):
    """both sides of the terms kernel's two thresholds (8 and 16 states) and of the avoidance walk's slices of 16 states: one
    slice, two with one state in the second, two full ones, three, four"""
    wide = K >= 17
    B = 200 if wide else 300          # (the one-thread program takes K^3 operations a step)
    g = chain(hml, ol.trace(B, min(K, 5), 7), K, every_position=True)
    assert g.num_blocks() == B
    check(hml, program, g, what=K, n_random=70 if wide else N_RANDOM)      # (with the edge regions: about 100)


@pytest.mark.parametrize("K,H", [(2, 1), (3, 1), (3, 2), (5, 32), (16, 32), (31, 32), (64, 15)])
def test_max_breaks(hml, program, K, H):
    """H = 1: the absorbing bin is bin 1.  K = 2 with H = 1: 4 cells on 64 lanes; K = 16 with H = 32: 528 cells, nine a lane at
    the most; 31 states with H = 32 and 64 with H = 15: the largest the rule allows, 1023 and 1024 cells"""
    assert cu.h_ok(K, H)
    wide = K >= 17
    B = 120 if wide else 300
    g = chain(hml, ol.trace(B, min(K, 5), 11), K, every_position=True)
    want, r, (start, end) = check(hml, program, g, H=H, what=(K, H), n_random=40 if wide else 500)
    if H == 1:
        whole = r["whole_state"].sum(axis=1)
        assert np.all(np.abs(r["hist"][:, 0] - whole) <= K * 2.0 ** -52)
        assert r["hist"][steps_of(g, start, end) > 0, 1].min() > 0.0


def test_more_regions_than_a_grid(hml, program):
    g = chain(hml, ol.trace(300, 3, 5), 3, every_position=True)
    want, r, (start, _) = check(hml, program, g, what="10 000", n_random=10000)
    assert len(start) > 2 * GRID


def test_blocks_of_many_positions(hml, program):
    g = chain(hml, ol.trace(30000, 5, 8), 5)
    assert g.num_blocks() < 30000
    check(hml, program, g)


def test_two_dimensions_two_parameters(hml, program):
    T = 600
    x = np.stack([ol.trace(T, 3, 1), ol.trace(T, 3, 2)], axis=1).reshape(-1)
    for every in (False, True):
        g = chain(hml, x, 4, dims=(2, 2), every_position=every)
        check(hml, program, g, what=every, n_random=500)


def test_self_transitions_off(hml, program):
    g = chain(hml, ol.trace(20000, 3, 5), 3, self_trans=False)
    check(hml, program, g, self_trans=False)


def test_zeros_in_A_and_pi(hml, program):
    """(the diagonal of A stays positive, as the smoothing's test explains)"""
    g = chain(hml, ol.trace(2000, 3, 9), 3, every_position=True)
    A = np.array([[0.5, 0.5, 0.0], [0.0, 0.5, 0.5], [0.75, 0.0, 0.25]], np.float32)
    g.set_parameters(np.array([-1.0, 0.05, 0.0, 0.05, 1.0, 0.05], np.float32), A, np.array([0.0, 1.0, 0.0], np.float32))
    want, r, (start, end) = check(hml, program, g)
    assert want["count_degenerate"] == 0
    # pi is all on state 1: a region from position 0 cannot avoid it
    assert not r["avoid"][start == 0, 1].any()


def test_a_block_no_path_reaches(hml, program):
    x = np.random.default_rng(2).normal(0, 0.3, 300).astype(np.float32)
    x[1:3] += 40.0
    g = chain(hml, x, 3, sweeps=1, every_position=True, self_trans=False)
    A = np.array([[0.5, 0.25, 0.25], [1.0, 0.0, 0.0], [0.25, 0.25, 0.5]], np.float32)
    g.set_parameters(np.array([0.0, 1.0, 0.0, 1.0, 40.0, 1.0], np.float32), A, np.array([0.0, 1.0, 0.0], np.float32))
    assert g.num_blocks() == 300
    want, r, _ = check(hml, program, g, self_trans=False, every_length=True)
    assert want["count_degenerate"] > 0
    t = g.posterior_count_terms()
    for a in (t["v"], t["rho"], r["hist"], r["whole_state"], r["avoid"]):
        assert not np.isnan(a).any() and np.isfinite(a).all()
    assert r["hist"].sum(axis=1).max() <= 1.0 + 300 * 3 * 2.0 ** -50       # mass is lost at such a boundary, never made


def planted_chain(hml, name):
    """the recipe on the device, as tests/test_gpu_infer_hostile.py puts it there: data loaded, every position a block, the
    planted parameters"""
    r = ic.CASES[name](None)
    assert r["block"] == 1
    g = hml.Chain(device=0, seed=3)
    if r["D"] > 1:
        g.set_dimensions(r["D"], r["P"])
    g.load(r["x"])
    g.set_model(r["K"], NIG4, self_trans=r["self_trans"])
    g.sample_prior()
    g.create_blocks(0.0)
    g.set_parameters(r["mean_var"], r["A"], r["pi"])
    assert g.num_blocks() == g.T == r["x"].size // r["D"]
    return g, r


@pytest.mark.parametrize("name", ic.DEVICE)
def test_planted_cases(hml, program, name):
    g, r = planted_chain(hml, name)
    want, got, _ = check(hml, program, g, self_trans=r["self_trans"], what=name, n_random=20)
    if "pair_degenerate" in ic.EXPECT[name]:
        assert want["count_degenerate"] > 0
    g.close()


@pytest.mark.parametrize("name", hi.family("scale", "offset", "depth", "spikes"))
def test_chains_on_hostile_inputs(hml, program, name):
    _, K, _ = hi.INPUTS[name]
    g = chain(hml, hi.data(name)[:20000], K, seed=hi.SEED[name], sweeps=5)
    check(hml, program, g, what=name, n_random=300)
    g.close()


def test_a_chain_that_halts_is_settled_first(hml, program):
    """a block capacity far below what the sweeps need: the chain halts; the call settles it, as hml_posterior does, and gives
    the words of the chain that never halted"""
    x = ol.trace(20000, 3, 7)
    g0 = chain(hml, x, 3, seed=9, sweeps=0)
    g1 = chain(hml, x, 3, seed=9, sweeps=0, options=(("max_blocks", 64),))
    for g in (g0, g1):
        g.iterate("F", 5, 0)
    start, end = [0, 10, 5000], [20000, 300, 9000]
    a, b = g0.posterior_region_counts(start, end), g1.posterior_region_counts(start, end)
    assert g1.stats()["buffer_growths"] > 0
    cu.same_regions(cu.region_words(a), cu.region_words(b))


# ---------------------------------------------------------------------------------------------- geometry is invisible
def weak_chain(hml, B=20000, K=5):
    """the decode's weakly separated trace: the smoothing's chunks depend on their warm-up"""
    rng = np.random.default_rng(17)
    st = np.cumsum(rng.random(B) < 0.01) % K
    x = (0.5 * st + rng.normal(0, 1, B)).astype(np.float32)
    g = chain(hml, x, K, sweeps=1, every_position=True)
    A = np.full((K, K), 0.0025, np.float32)
    np.fill_diagonal(A, 0.99)
    mv = np.stack([0.5 * np.arange(K), np.ones(K)], 1).ravel().astype(np.float32)
    g.set_parameters(mv, A, np.full(K, 0.2, np.float32))
    assert g.num_blocks() == B
    return g


def test_geometry_is_invisible(hml, program):
    """the words do not move under geometries of the smoothing pass that make the repair and the single lane run"""
    g = weak_chain(hml)
    check(hml, program, g, n_random=300)
    start, end = pz.edge_regions(g.blocks(), np.random.default_rng(17), 500)
    short = steps_of(g, start, end) <= 2000          # (the whole-trace regions: once, in check above)
    start, end = start[short], end[short]
    flat = lambda d: [np.asarray(v).tobytes() for v in d.values()]
    first = flat(g.posterior_count_terms()) + flat(g.posterior_region_counts(start, end, 4))
    seen_repair = seen_serial = False
    for W, L, rounds in [(1, 4, 0), (1, 64, 1), (4, 512, 8), (1024, 64, 8), (1, 512, 2)]:
        g.set_option("posterior_W", W)
        g.set_option("posterior_L", L)
        g.set_option("posterior_rounds", rounds)
        got = flat(g.posterior_count_terms()) + flat(g.posterior_region_counts(start, end, 4))
        assert got == first, (W, L, rounds)
        info = g.posterior_info()                 # the smoothing pass behind the last call
        assert info["W"] == W and info["L"] == L
        seen_repair |= info["stale_fwd"] > 0 and info["stale_bwd"] > 0
        seen_serial |= info["serial_chunks"] > 0
    assert seen_repair and seen_serial


# ---------------------------------------------------------------------------------------------- against the other exact read-outs
def test_against_the_pairwise_read_outs(hml, program):
    """whole_state and hist[0] against hml_posterior_regions' whole_state and whole within twice its quantisation bound,
    (be - ba) 2^-23 relative; where that read-out's capped cost makes a value exactly 0, this one is below 1e-300.  Where the
    restatement shows an empty absorbing bin (hist[H] < 1e-12), the histogram's mean against expected_breaks within
    (be - ba) 2^-33 + H 1e-12 + 1e-12.  H = 16 and 1000 regions of a geometric number of blocks, five on average, behind the
    edge regions: 0.8^16 = 3 % of them span more than 16 blocks, the others cannot hold 16 breakpoints, so that at least nine
    regions in ten have an empty absorbing bin"""
    H, B = 16, 2000
    g = chain(hml, ol.trace(B, 3, 21), 3, every_position=True)
    assert g.num_blocks() == B
    rng = np.random.default_rng(8)
    start, end = pz.edge_regions(g.blocks(), rng, 0)
    a = rng.integers(0, B, 1000)
    e = np.minimum(a + rng.geometric(0.2, 1000), B)          # (a block a position)
    regions = np.concatenate([start, a.astype(np.uint32)]), np.concatenate([end, e.astype(np.uint32)])
    want, r, (start, end) = check(hml, program, g, H=H, regions=regions)
    pair = g.posterior_regions(start, end)
    n = steps_of(g, start, end).astype(np.float64)
    for new, old, what in ((r["whole_state"], pair["whole_state"], "whole_state"), (r["hist"][:, 0], pair["whole"], "whole")):
        new, old = np.asarray(new).reshape(len(n), -1), np.asarray(old).reshape(len(n), -1)
        zero = old == 0.0
        assert np.all(new[zero] < 1e-300), what
        err, bound = np.abs(new - old), 2.0 * n[:, None] * 2.0 ** -23 * new
        print("%s: %d values, %d exactly 0 there; worst %.3f of the bound" % (what, new.size, zero.sum(), np.max(err[~zero] / np.maximum(bound[~zero], 1e-300))))
        assert np.all(err[~zero] <= bound[~zero]), what
    hist = want["hist"].view(np.float64)
    empty = hist[:, H] < 1e-12
    print("regions with an empty absorbing bin: %d of %d" % (empty.sum(), len(empty)))
    assert empty.mean() >= 0.9
    mean = (r["hist"] * np.arange(H + 1)).sum(axis=1)
    margin = n * 2.0 ** -33 + H * 1e-12 + 1e-12
    print("mean against expected_breaks: worst %.3g of the margin" % np.max(np.abs(mean - pair["expected_breaks"])[empty] / margin[empty]))
    assert np.all(np.abs(mean - pair["expected_breaks"])[empty] <= margin[empty])


def within_bernstein(count, p, R, what):
    count, p = np.asarray(count, np.float64).ravel(), np.asarray(p, np.float64).ravel()
    dev, bound = np.abs(count - R * p), su.bernstein(R, p)
    worst = int(np.argmax(dev / bound))
    print("%s: %d cells, worst %.2f of the bound" % (what, count.size, dev[worst] / bound[worst]))
    assert np.all(dev <= bound), (what, worst, count[worst], R * p[worst])


@pytest.mark.parametrize("kind", ["separated", "weak"])
def test_against_the_sample(hml, kind):
    """4096 draws of hml_posterior_sample_regions: every bin of the histogram, and the whole-state counts, within Bernstein's
    bound at delta = 1e-12 of the exact probabilities"""
    R, B, H = 4096, 2000, 3
    g = chain(hml, ol.trace(B, 3, 21), 3, every_position=True) if kind == "separated" else weak_chain(hml, B)
    assert g.num_blocks() == B
    start, end = pz.edge_regions(g.blocks(), np.random.default_rng(6), n_random=40)
    exact = g.posterior_region_counts(start, end, H)
    assert exact["count_degenerate"] == 0
    reg = g.posterior_sample_regions(start, end, R, seed=31, max_breaks=H)
    within_bernstein(reg["hist"], exact["hist"], R, kind + " hist")
    within_bernstein(reg["whole_state"], exact["whole_state"], R, kind + " whole_state")
    if kind == "weak":
        assert exact["hist"][:, H].max() > 0.5          # the absorbing bin is compared too


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals(hml):
    g = chain(hml, ol.trace(5000, 3, 11), 3, sweeps=0)
    for call in (lambda: g.posterior_region_counts([0], [5]), g.posterior_count_terms):
        with pytest.raises(hml.HmlError) as e:
            call()                        # no blocks yet
        assert e.value.code == 1 and "no blocks yet: run a sweep or hml_create_blocks first" in str(e.value)
    with pytest.raises(hml.HmlError) as e:
        g.posterior_counts_info()
    assert "nothing was computed yet" in str(e.value)
    g.create_blocks(0.5)
    flat = lambda d: [np.asarray(v).tobytes() for v in d.values()]
    good = g.posterior_region_counts([0, 7], [5000, 300], 4)
    info = g.posterior_counts_info()
    state = (g.states().tobytes(), g.theta().tobytes(), g.blocks().tobytes())
    assert info["regions"] == 2
    for H in (0, 33, 2 ** 32 - 1):
        with pytest.raises(hml.HmlError) as e:
            g.posterior_region_counts([0], [5], H)
        assert e.value.code == 1 and "max_breaks must be 1 ... 32 with K (max_breaks + 1) <= 1024" in str(e.value), H
    for start, end in (([0, 5], [1, 5]), ([0, 0], [1, 5001]), ([0, 7], [1, 3]), ([0, 5000], [1, 5001])):
        with pytest.raises(hml.HmlError) as e:
            g.posterior_region_counts(start, end)
        assert e.value.code == 1 and "region 1 is" in str(e.value) and "it must hold a position and end at or before T" in str(e.value)
    # nothing has changed: the numbers about the last call, the chain, the next answer
    assert g.posterior_counts_info() == info
    assert (g.states().tobytes(), g.theta().tobytes(), g.blocks().tobytes()) == state
    assert flat(g.posterior_region_counts([0, 7], [5000, 300], 4)) == flat(good)
    empty = g.posterior_region_counts([], [])          # n = 0 succeeds
    assert empty["hist"].shape == (0, 9) and empty["avoid"].shape == (0, 3) and empty["count_degenerate"] == good["count_degenerate"]
    assert g.posterior_counts_info() == dict(regions=0, steps=0, longest=0)
    # 64 states: 15 is the largest
    g64 = chain(hml, ol.trace(200, 5, 7), 64, every_position=True, sweeps=1)
    with pytest.raises(hml.HmlError) as e:
        g64.posterior_region_counts([0], [5], 16)
    assert e.value.code == 1 and "K (max_breaks + 1) <= 1024" in str(e.value) and "K = 64" in str(e.value)
    assert g64.posterior_region_counts([0], [5], 15)["hist"].shape == (1, 16)


def test_counts_info(hml):
    """the regions, the sum of be - ba and the largest, against the blocks in Python"""
    g = chain(hml, ol.trace(30000, 3, 8), 3)
    start, end = pz.edge_regions(g.blocks(), np.random.default_rng(4), 5000)
    n = steps_of(g, start, end)
    g.posterior_region_counts(start, end, 2)
    assert g.posterior_counts_info() == dict(regions=len(start), steps=int(n.sum()), longest=int(n.max()))
    g.posterior_region_counts([3], [4], 2)
    assert g.posterior_counts_info() == dict(regions=1, steps=0, longest=0)


# ---------------------------------------------------------------------------------------------- memory, side effects
def test_calls_keep_no_device_memory_and_survive_failed_allocations(hml):
    g = chain(hml, ol.trace(5000, 3, 3), 3, every_position=True)
    g.set_option("posterior_W", 1)      # (stale chunks: the repair kernels run too)
    rng = np.random.default_rng(1)
    start, end = pz.edge_regions(g.blocks(), rng, 100)
    gc.collect()      # (chains that earlier tests dropped without closing go first: the totals below are this test's alone)
    before = hml.device_memory_live()
    flat = lambda d: [np.asarray(v).tobytes() for v in d.values()]
    calls = {"posterior_region_counts": lambda: g.posterior_region_counts(start, end, 4), "posterior_count_terms": g.posterior_count_terms}
    for name, call in calls.items():
        hml.debug_fail_allocation(10 ** 9)
        good = call()
        n_alloc = hml.debug_fail_allocation(0)
        assert n_alloc >= 5 and hml.device_memory_live() == before, name
        for n in range(1, n_alloc + 1):
            hml.debug_fail_allocation(n)
            with pytest.raises(hml.HmlError) as e:
                call()
            hml.debug_fail_allocation(0)
            assert e.value.code == 2 and "out of memory" in str(e.value), (name, n)
            assert hml.device_memory_live() == before, (name, n)
        assert flat(call()) == flat(good) and hml.device_memory_live() == before, name


def test_under_guard_bands_and_poison(hml, program):
    hml.debug_guard_allocations(4096, True)
    try:
        g = chain(hml, ol.trace(300, 5, 4), 17, every_position=True)
        check(hml, program, g, what="guarded", n_random=200, every_length=True)
        g.set_option("posterior_W", 1)
        g.set_option("posterior_L", 4)
        g.set_option("posterior_rounds", 1)
        check(hml, program, g, H=32, what="guarded, repairs", n_random=50)
        del g
        gc.collect()
        assert hml.debug_check_guards() == {"damaged": 0}
    finally:
        hml.debug_guard_allocations(0)


def test_the_calls_leave_the_chain_alone(hml):
    x = ol.trace(40000, 3, 13)

    def run(call):
        g = chain(hml, x, 3, seed=5, sweeps=0)
        g.iterate("F", 6, 2)
        if call:
            g.posterior_region_counts([0, 10, 10], [40000, 20, 20])
        g.iterate("F", 6, 2)
        if call:
            g.set_option("posterior_W", 1)
            g.posterior_count_terms()
            g.posterior_region_counts([5], [6], 1)
        g.iterate("M", 2, 1)
        g.sync()
        seg, cnt = g.marginals_rle()
        return g.states(), g.theta(), g.transitions(), seg, cnt, g.blocks()

    a, b = run(False), run(True)
    flat = lambda r: [np.asarray(v).tobytes() for part in r for v in (part if isinstance(part, tuple) else (part,))]
    assert flat(a) == flat(b)

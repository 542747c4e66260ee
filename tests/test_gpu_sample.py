"""Path sampling on the device (hml_posterior_sample ... hml_set_sample_batch_bytes, include/hml.h) against the restatement for
one host thread, tests/fixtures/sample_ref_main.cpp over hammlet_amd/csrc/hml_sample_ref.h, which is fed the GPU's own
block_stats(), blocks(), theta() and transitions().  Every output is an integer - paths, segments, scores, change, state and
region counts, the degenerate count - and is compared as such: there is no tolerance in the word comparisons of this file.

The last section compares the sample with the exact read-outs (gamma of hml_posterior, p of hml_posterior_pair_terms, whole and
whole_state of hml_posterior_regions) within Bernstein's bound at delta = 1e-12 per cell, |count - R p| <= L/3 + sqrt(L^2/9 +
2 R p (1 - p) L), L = ln(2 / delta) (tests/test_sample_cpu.py): derived, not measured."""
import gc
import itertools
import os

import numpy as np
import pytest

from tests import hostile_inputs as hi
from tests import oracle_lib as ol
from tests import pairs_util as pr
from tests import sample_util as su
from tests.test_gpu_posterior import chain, weak_chain

pytestmark = pytest.mark.gpu

DEFAULT_L, DEFAULT_W = 256, 256
H = 3


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("sample_ref")
    return su.build_programs(d, sanitized=False)["plain"], str(d)


def reference(program, g, count, seed, first=0, self_trans=True, regions=((), ())):
    exe, d = program
    return su.run_program(exe, su.chain_case(g, self_trans), first, count, seed, regions[0], regions[1], H, paths_file=os.path.join(d, "paths"))


def check_sample(g, want, count, seed, first=0, what=None):
    got = g.posterior_sample(count, seed=seed, first=first, paths=True, state_counts=True)
    assert np.array_equal(got["paths"], want["paths"]), what
    su.same(got, want, su.COUNT_KEYS, what)
    return got


def check(program, g, count, seed=7, first=0, self_trans=True, what=None, degenerate=False):
    """paths and every count of the sample and of the regions; the invariants, with the score bound against hml_viterbi"""
    rng = np.random.default_rng(5)
    regions = pr.edge_regions(g.blocks(), rng, n_random=3)
    want = reference(program, g, count, seed, first, self_trans, regions)
    got = check_sample(g, want, count, seed, first, what)
    reg = g.posterior_sample_regions(regions[0], regions[1], count, seed=seed, first=first, max_breaks=H)
    su.same(reg, want, su.REGION_KEYS, what)
    su.same(reg, su.region_counts(got["paths"], g.K, g.blocks(), regions[0], regions[1], H), su.REGION_KEYS, what)
    A, pi = g.transitions()
    su.invariants(got, g.K, count, g.viterbi()[2][0], *(() if degenerate else (A, pi)))
    info = g.posterior_sample_info()
    assert info["draws"] == count and info["chunks"] == (g.num_blocks() + info["L"] - 1) // info["L"]
    return want, got


@pytest.mark.parametrize("T", [1, 2, 3, 16, 65])
def test_tiny_traces(hml, program, T):
    if T == 1:
        g = hml.Chain(device=0, seed=12)                  # one block
        g.load(np.array([0.3], np.float32))
        g.set_model(2, np.array([2.0, 1.0, 0.0, 1.0], np.float32))
        g.sample_prior()
        g.create_blocks(1.0)
        assert g.num_blocks() == 1
    else:
        g = chain(hml, ol.trace(1000, 3, 2)[:T].copy(), 2, seed=12, sweeps=10)
    want, got = check(program, g, 65, what=T)
    assert want["sample_degenerate"] == 0
    info = g.posterior_sample_info()
    assert info["L"] == DEFAULT_L and info["W"] == DEFAULT_W and info["groups"] == 1 and info["group_size"] == 65


@pytest.mark.parametrize("B,count", [(64 * DEFAULT_L - 1, 1), (64 * DEFAULT_L, 63), (64 * DEFAULT_L + 1, 64), (70000, 130)])
def test_every_position_a_block(hml, program, B, count):
    g = chain(hml, ol.trace(B, 5, 4), 5, every_position=True)
    assert g.num_blocks() == B
    check(program, g, count, what=B)


@pytest.mark.parametrize("K", [2, 8, 9, 16, 17, 64])
def test_numbers_of_states(hml, program, K):
    g = chain(hml, ol.trace(3000, min(K, 5), 7), K, every_position=True)
    check(program, g, 65, what=K)


def test_two_dimensions_two_parameters(hml, program):
    T = 4096
    x = np.stack([ol.trace(T, 3, 1), ol.trace(T, 3, 2)], axis=1).reshape(-1)
    g = chain(hml, x, 4, dims=(2, 2), every_position=True)
    check(program, g, 64)


@pytest.mark.parametrize("name", hi.family("ties"))
def test_integer_data_full_of_ties(hml, program, name):
    fn, K, _ = hi.INPUTS[name]
    g = chain(hml, hi.data(name)[:20000], K, seed=hi.SEED[name], sweeps=5)
    check(program, g, 65, what=name)


def test_self_transitions_off(hml, program):
    g = chain(hml, ol.trace(20000, 3, 5), 3, self_trans=False)
    check(program, g, 65, self_trans=False)


def test_compat_context(hml, program):
    g = chain(hml, ol.trace(20000, 3, 6), 3, options=[("compat", 1)], sweeps=5)
    g.create_blocks(g.threshold())
    check(program, g, 65, what="compat")


def zeros_chain(hml):
    g = chain(hml, ol.trace(20000, 3, 9), 3, every_position=True)
    A = np.array([[0.5, 0.5, 0.0], [0.0, 0.5, 0.5], [0.75, 0.0, 0.25]], np.float32)
    g.set_parameters(np.array([-1.0, 0.05, 0.0, 0.05, 1.0, 0.05], np.float32), A, np.array([0.0, 1.0, 0.0], np.float32))
    return g


def test_zeros_in_A_and_pi(hml, program):
    want, got = check(program, zeros_chain(hml), 130)
    assert want["sample_degenerate"] == 0 and np.all(got["paths"][:, 0] == 1)


def unreachable_chain(hml):
    """pi = (0, 1, 0), state 1 leads to state 0 alone, and position 1 lies 40 sigma from state 0's level: c_1 = 0"""
    x = np.random.default_rng(2).normal(0, 0.3, 300).astype(np.float32)
    x[1:3] += 40.0
    g = chain(hml, x, 3, sweeps=1, every_position=True, self_trans=False)
    A = np.array([[0.5, 0.25, 0.25], [1.0, 0.0, 0.0], [0.25, 0.25, 0.5]], np.float32)
    g.set_parameters(np.array([0.0, 1.0, 0.0, 1.0, 40.0, 1.0], np.float32), A, np.array([0.0, 1.0, 0.0], np.float32))
    return g


def test_a_block_no_path_reaches(hml, program):
    want, got = check(program, unreachable_chain(hml), 130, self_trans=False, degenerate=True)
    assert want["sample_degenerate"] == int((got["paths"][:, 1] == 2).sum()) > 0


def test_refusals(hml):
    g = chain(hml, ol.trace(5000, 3, 11), 3, sweeps=0)
    for call in (lambda: g.posterior_sample(4), lambda: g.posterior_sample_regions([0], [5], 4)):
        with pytest.raises(hml.HmlError) as e:
            call()                        # no blocks yet
        assert "no blocks yet: run a sweep or hml_create_blocks first" in str(e.value)
    with pytest.raises(hml.HmlError):
        g.posterior_sample_info()
    g.create_blocks(0.5)
    for bad in (dict(count=0), dict(count=2 ** 24 + 1), dict(count=2, first=2 ** 48 - 1)):
        with pytest.raises(hml.HmlError) as e:
            g.posterior_sample(**bad)
        assert e.value.code == 1, bad
    for start, end in (([5], [5]), ([0], [5001]), ([7], [3])):
        with pytest.raises(hml.HmlError) as e:
            g.posterior_sample_regions(start, end, 4)
        assert "it must hold a position and end at or before T" in str(e.value)
    with pytest.raises(hml.HmlError):
        g.posterior_sample_regions([0], [5], 4, max_breaks=0)
    r = g.posterior_sample_regions([], [], 4)       # n = 0
    assert r["hist"].shape == (0, 9)
    for name, value in (("sample_W", -1), ("sample_L", (1 << 20) + 1), ("sample_rounds", 17)):
        with pytest.raises(hml.HmlError):
            g.set_option(name, value)


# ---------------------------------------------------------------------------------------------- geometry is invisible
@pytest.fixture(scope="module")
def weak(hml, program):
    """the weakly separated chain of tests/test_gpu_posterior.py and the restatement's words for 130 draws of it, computed once"""
    g = weak_chain(hml)
    rng = np.random.default_rng(5)
    regions = pr.edge_regions(g.blocks(), rng, n_random=20)
    want = reference(program, g, 130, 11, regions=regions)
    check_sample(g, want, 130, 11, what="default")
    info = g.posterior_sample_info()
    print("default geometry: %s" % info)
    return g, want, regions


@pytest.mark.parametrize("W", [1, 4, 16, 1024])
def test_geometry_is_invisible(weak, W):
    g, want, _ = weak
    B = g.num_blocks()
    for L, rounds in itertools.product((4, 64, 512), (0, 1, 8)):
        g.set_option("sample_W", W)
        g.set_option("sample_L", L)
        g.set_option("sample_rounds", rounds)
        check_sample(g, want, 130, 11, what=(W, L, rounds))
        info = g.posterior_sample_info()
        print("W %4d L %3d rounds %d: %s" % (W, L, rounds, info))
        chunks = (B + L - 1) // L
        assert info["W"] == W and info["L"] == L and info["chunks"] == chunks and info["rounds"] <= rounds
        assert info["stale_first"] <= 130 * (chunks - 1) and info["serial_chunks"] <= 130 * (chunks - 1)
        if W == 1:
            assert info["stale_first"] > 0, (L, rounds)                # the repair ran ...
            if rounds == 0:
                assert info["serial_chunks"] > 0, L                   # ... and without rounds all of it on the finishing lanes
            else:
                assert info["rounds"] > 0, L
        if info["stale_first"] == 0 or rounds == 0:
            assert info["rounds"] == 0
        if info["stale_first"] == 0:
            assert info["serial_chunks"] == 0
    for name in ("sample_W", "sample_L"):
        g.set_option(name, 0)
    g.set_option("sample_rounds", 8)


def test_one_chunk_and_regions_under_a_geometry_that_repairs(weak):
    g, want, regions = weak
    g.set_option("sample_L", 32768)
    check_sample(g, want, 130, 11, what="one chunk")
    info = g.posterior_sample_info()
    assert info["chunks"] == 1 and info["stale_first"] == 0 and info["serial_chunks"] == 0 and info["rounds"] == 0
    g.set_option("sample_L", 4)
    g.set_option("sample_W", 1)
    g.set_option("sample_rounds", 1)
    reg = g.posterior_sample_regions(regions[0], regions[1], 130, seed=11, max_breaks=H)
    su.same(reg, want, su.REGION_KEYS, "regions")
    assert g.posterior_sample_info()["stale_first"] > 0
    for name in ("sample_W", "sample_L"):
        g.set_option(name, 0)
    g.set_option("sample_rounds", 8)


# ---------------------------------------------------------------------------------------------- grouping and windows
def test_groups_and_windows(weak):
    g, want, regions = weak
    B = g.num_blocks()
    chunks = (B + DEFAULT_L - 1) // DEFAULT_L
    per_draw = 2 * B + 10 * chunks + 16                   # with paths (include/hml.h)
    for size in (1, 3):
        g.set_sample_batch_bytes(size * per_draw + per_draw // 2)
        check_sample(g, want, 130, 11, what=size)
        info = g.posterior_sample_info()
        assert info["group_size"] == size and info["groups"] == (130 + size - 1) // size, info
        reg = g.posterior_sample_regions(regions[0], regions[1], 130, seed=11, max_breaks=H)
        su.same(reg, want, su.REGION_KEYS, size)
        assert g.posterior_sample_info()["groups"] > 1
    g.set_sample_batch_bytes(1)                           # at least one draw a group
    part = g.posterior_sample(4, seed=11, first=5, paths=True)
    assert g.posterior_sample_info()["group_size"] == 1
    g.set_sample_batch_bytes(0)
    assert np.array_equal(part["paths"], want["paths"][5:9])
    assert np.array_equal(part["segments"].astype(np.int64), want["segments"][5:9]) and np.array_equal(part["score_fixed"], want["score_fixed"][5:9])
    again = g.posterior_sample(4, seed=11, first=5, paths=True)
    assert g.posterior_sample_info()["groups"] == 1 and np.array_equal(again["paths"], part["paths"])
    other = g.posterior_sample(4, seed=12, first=5, paths=True)
    assert not np.array_equal(other["paths"], part["paths"])


# ---------------------------------------------------------------------------------------------- against the exact read-outs
def within_bernstein(count, p, R, what):
    count, p = np.asarray(count, np.float64).ravel(), np.asarray(p, np.float64).ravel()
    dev, bound = np.abs(count - R * p), su.bernstein(R, p)
    worst = int(np.argmax(dev / bound))
    print("%s: %d cells, worst %.2f of the bound" % (what, count.size, dev[worst] / bound[worst]))
    assert np.all(dev <= bound), (what, worst, count[worst], R * p[worst])


@pytest.mark.parametrize("kind", ["separated", "weak"])
def test_against_the_exact_read_outs(hml, kind):
    R, B = 4096, 2000
    if kind == "separated":
        g = chain(hml, ol.trace(B, 3, 21), 3, every_position=True)
    else:
        rng = np.random.default_rng(23)
        st = np.cumsum(rng.random(B) < 0.01) % 5
        g = chain(hml, (0.5 * st + rng.normal(0, 1, B)).astype(np.float32), 5, sweeps=1, every_position=True)
        A = np.full((5, 5), 0.0025, np.float32)
        np.fill_diagonal(A, 0.99)
        g.set_parameters(np.stack([0.5 * np.arange(5), np.ones(5)], 1).ravel().astype(np.float32), A, np.full(5, 0.2, np.float32))
    assert g.num_blocks() == B
    s = g.posterior_sample(R, seed=31, state_counts=True)
    gamma, _, degenerate = g.posterior()
    assert degenerate == 0 and s["sample_degenerate"] == 0
    within_bernstein(s["state_count"], gamma, R, kind + " state_count against gamma")
    within_bernstein(s["change_count"], g.posterior_pair_terms()["p"], R, kind + " change_count against p")
    start, end = pr.edge_regions(g.blocks(), np.random.default_rng(6), n_random=40)
    exact = g.posterior_regions(start, end)
    reg = g.posterior_sample_regions(start, end, R, seed=31, max_breaks=H)
    within_bernstein(reg["hist"][:, 0], exact["whole"], R, kind + " hist[0] against whole")
    within_bernstein(reg["whole_state"], exact["whole_state"], R, kind + " whole_state")
    assert np.all(reg["hist"].sum(1) == R) and np.all(reg["whole_state"].sum(1) == reg["hist"][:, 0])


# ---------------------------------------------------------------------------------------------- memory
def test_a_call_keeps_no_device_memory_and_survives_failed_allocations(hml):
    g = chain(hml, ol.trace(5000, 3, 3), 3, every_position=True)
    g.set_option("sample_W", 1)      # (stale chunks: the repair kernels run too)
    g.set_option("posterior_W", 1)
    gc.collect()      # (chains that earlier tests dropped without closing go first: the totals below are this test's alone)
    before = hml.device_memory_live()
    calls = {"sample": lambda: g.posterior_sample(70, seed=3, paths=True, state_counts=True),
             "regions": lambda: g.posterior_sample_regions([0, 100], [5000, 2000], 70, seed=3)}
    for name, call in calls.items():
        hml.debug_fail_allocation(10 ** 9)
        good = call()
        n_alloc = hml.debug_fail_allocation(0)
        assert n_alloc >= 10 and hml.device_memory_live() == before, name
        for n in range(1, n_alloc + 1):
            hml.debug_fail_allocation(n)
            with pytest.raises(hml.HmlError) as e:
                call()
            hml.debug_fail_allocation(0)
            assert e.value.code == 2 and "out of memory" in str(e.value), (name, n)
            assert hml.device_memory_live() == before, (name, n)
        again = call()                # the next call succeeds, with the same answer
        assert all(np.array_equal(again[k], good[k]) for k in good) and hml.device_memory_live() == before, name


def test_under_guard_bands_and_poison(hml, program):
    hml.debug_guard_allocations(4096, True)
    try:
        g = chain(hml, ol.trace(64 * DEFAULT_L + 1, 5, 4), 5, every_position=True)
        check(program, g, 65, what="guarded")
        g.set_option("sample_W", 1)
        g.set_option("sample_L", 4)
        g.set_option("sample_rounds", 1)
        g.set_sample_batch_bytes(40 * (2 * g.num_blocks() + 10 * ((g.num_blocks() + 3) // 4) + 16))
        check(program, g, 65, what="guarded, repairs, two groups")
        assert g.posterior_sample_info()["groups"] == 2
        check(program, unreachable_chain(hml), 130, self_trans=False, degenerate=True, what="guarded, unreachable")
        del g
        gc.collect()
        assert hml.debug_check_guards() == {"damaged": 0}
    finally:
        hml.debug_guard_allocations(0)

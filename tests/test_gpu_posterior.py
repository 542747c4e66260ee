"""Smoothing on the device (hml_posterior ... hml_posterior_info, include/hml.h) against the restatement for one host thread,
tests/fixtures/posterior_ref_main.cpp over hammlet_amd/csrc/hml_posterior_ref.h, which is fed the GPU's own block_stats(),
blocks(), theta() and transitions():
  (a) posterior_terms() equals its e, m, alpha, c and beta word for word;
  (b) posterior() equals its gamma, log-likelihood and degenerate count, posterior_rle() its runs and confidences.
Floats are compared as their 32-bit, doubles as their 64-bit words: there is no tolerance anywhere in this file."""
import gc
import itertools
import time

import numpy as np
import pytest

from tests import hostile_inputs as hi
from tests import oracle_lib as ol
from tests import posterior_util as pu

pytestmark = pytest.mark.gpu

DEFAULT_L, DEFAULT_W = 64, 256


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return pu.build_programs(tmp_path_factory.mktemp("posterior_ref"), sanitized=False)["plain"]


def reference(program, g, self_trans=True):
    return pu.run_case(program, pu.chain_case(g, self_trans))


def check_results(g, want, what=None):
    """(b): gamma, log-likelihood, degenerate count, runs over positions with their confidences"""
    gamma, loglik, degenerate = g.posterior()
    assert np.array_equal(pu.words(gamma), want["gamma"].ravel()), what
    assert pu.words([loglik])[0] == want["loglik"][0] and degenerate == want["degenerate"], what
    run_len, run_state, run_conf = g.posterior_rle()
    assert np.array_equal(run_len, want["run_len"].astype(np.uint64)) and np.array_equal(run_state, want["run_state"]), what
    assert np.array_equal(pu.words(run_conf), want["run_conf"]), what
    assert int(run_len.sum()) == g.T and np.all(run_state[1:] != run_state[:-1])
    return gamma, loglik


def check(program, g, self_trans=True, what=None):
    """(a) and (b)"""
    want = reference(program, g, self_trans)
    e, m, alpha, c, beta = g.posterior_terms()
    assert np.array_equal(pu.words32(e), want["e"].ravel()), what
    assert np.array_equal(pu.words32(m), want["m"]), what
    assert np.array_equal(pu.words(alpha), want["alpha"].ravel()), what
    assert np.array_equal(pu.words(c), want["c"]), what
    assert np.array_equal(pu.words(beta), want["beta"].ravel()), what
    check_results(g, want, what)
    return want


def chain(hml, x, K, seed=3, sweeps=3, options=(), dims=None, self_trans=True, every_position=False):
    g = hml.Chain(device=0, seed=seed)
    for name, value in options:
        g.set_option(name, value)
    if dims:
        g.set_dimensions(*dims)
    g.load(x)
    if every_position:
        g.scale_weights(1e9)
    g.set_model(K, g.autoprior(0.2, 0.9), self_trans=self_trans)
    g.sample_prior()
    if sweeps:
        g.iterate("F", sweeps, 0)
        g.sync()
    return g


@pytest.mark.parametrize("T", [2, 3, 16, 65])
def test_tiny_traces(hml, program, T):
    g = chain(hml, ol.trace(1000, 3, 2)[:T].copy(), 2, seed=12, sweeps=10)
    want = check(program, g, what=T)
    assert want["degenerate"] == 0
    info = g.posterior_info()
    assert info["chunks"] == (g.num_blocks() + DEFAULT_L - 1) // DEFAULT_L and info["L"] == DEFAULT_L and info["W"] == DEFAULT_W


@pytest.mark.parametrize("B", [64 * DEFAULT_L - 1, 64 * DEFAULT_L, 64 * DEFAULT_L + 1, 70000])
def test_every_position_a_block(hml, program, B):
    g = chain(hml, ol.trace(B, 5, 4), 5, every_position=True)
    assert g.num_blocks() == B
    want = check(program, g, what=B)
    assert want["degenerate"] == 0 and np.isfinite(want["loglik"].view(np.float64)[0])
    assert g.posterior_info()["chunks"] == (B + DEFAULT_L - 1) // DEFAULT_L


@pytest.mark.parametrize("K", [2, 5, 10, 16, 20, 64])
def test_numbers_of_states(hml, program, K):
    g = chain(hml, ol.trace(3000, min(K, 5), 7), K, every_position=True)
    check(program, g, what=K)
    g = chain(hml, ol.trace(30000, min(K, 5), 8), K)
    check(program, g, what=K)


def test_two_dimensions_two_parameters(hml, program):
    T = 4096
    x = np.stack([ol.trace(T, 3, 1), ol.trace(T, 3, 2)], axis=1).reshape(-1)
    for every in (False, True):
        g = chain(hml, x, 4, dims=(2, 2), every_position=every)
        check(program, g, what=every)


@pytest.mark.parametrize("name", hi.family("ties"))
def test_integer_data_full_of_ties(hml, program, name):
    fn, K, _ = hi.INPUTS[name]
    g = chain(hml, hi.data(name)[:20000], K, seed=hi.SEED[name], sweeps=5)
    check(program, g, what=name)


def test_self_transitions_off(hml, program):
    g = chain(hml, ol.trace(20000, 3, 5), 3, self_trans=False)
    check(program, g, self_trans=False)


def test_compat_context_gives_the_same_tables_and_posteriors(hml, program):
    x = ol.trace(20000, 3, 6)
    c = chain(hml, x, 3, options=[("compat", 1)], sweeps=5)
    A, pi = c.transitions()
    d = chain(hml, x, 3, sweeps=0)
    d.set_parameters(c.theta(), A, pi)
    thr = c.threshold()
    c.create_blocks(thr)
    d.create_blocks(thr)
    assert np.array_equal(c.blocks(), d.blocks())
    want = check(program, c, what="compat")
    for a, b in zip(c.posterior_terms(), d.posterior_terms()):
        assert a.tobytes() == b.tobytes()
    check_results(d, want, "default")


def test_after_set_parameters_with_zeros_in_A_and_pi(hml, program):
    """(the diagonal of A stays positive: with self-transitions a block of one position in a state with A_jj = 0 has the term
    0 x -inf, which is not a number - and whose sign no standard fixes)"""
    g = chain(hml, ol.trace(20000, 3, 9), 3, every_position=True)
    A = np.array([[0.5, 0.5, 0.0], [0.0, 0.5, 0.5], [0.75, 0.0, 0.25]], np.float32)
    pi = np.array([0.0, 1.0, 0.0], np.float32)
    g.set_parameters(np.array([-1.0, 0.05, 0.0, 0.05, 1.0, 0.05], np.float32), A, pi)
    want = check(program, g)
    gamma = want["gamma"].view(np.float64)
    assert gamma[0, 0] == 0.0 and gamma[0, 2] == 0.0 and gamma[0, 1] == 1.0 and gamma[1, 0] == 0.0


def test_a_block_no_path_reaches(hml, program):
    """pi = (0, 1, 0), state 1 leads to state 0 alone, and position 1 lies 40 sigma from state 0's level: c_1 = 0"""
    x = np.random.default_rng(2).normal(0, 0.3, 300).astype(np.float32)
    x[1:3] += 40.0
    g = chain(hml, x, 3, sweeps=1, every_position=True, self_trans=False)
    A = np.array([[0.5, 0.25, 0.25], [1.0, 0.0, 0.0], [0.25, 0.25, 0.5]], np.float32)
    g.set_parameters(np.array([0.0, 1.0, 0.0, 1.0, 40.0, 1.0], np.float32), A, np.array([0.0, 1.0, 0.0], np.float32))
    assert g.num_blocks() == 300
    want = check(program, g, self_trans=False)
    gamma, loglik, degenerate = g.posterior()
    assert degenerate == 1 and loglik == -np.inf and not np.isnan(gamma).any()


def test_after_create_blocks_on_a_chain_that_never_iterated(hml, program):
    g = chain(hml, ol.trace(50000, 3, 11), 3, sweeps=0)
    for call in (g.posterior, g.posterior_rle, g.posterior_terms):
        with pytest.raises(hml.HmlError) as e:
            call()                        # no blocks yet
        assert "no blocks yet: run a sweep or hml_create_blocks first" in str(e.value)
    with pytest.raises(hml.HmlError):
        g.posterior_info()
    for thr in (0.5, 3.0):
        g.create_blocks(thr)
        check(program, g, what=thr)


# ---------------------------------------------------------------------------------------------- geometry is invisible
WEAK_B = 20000


def weak_chain(hml):
    """five states 0.5 sigma apart, sticky A, every position a block"""
    rng = np.random.default_rng(17)
    st = np.cumsum(rng.random(WEAK_B) < 0.01) % 5
    x = (0.5 * st + rng.normal(0, 1, WEAK_B)).astype(np.float32)
    g = chain(hml, x, 5, sweeps=1, every_position=True)
    A = np.full((5, 5), 0.0025, np.float32)
    np.fill_diagonal(A, 0.99)
    mv = np.stack([0.5 * np.arange(5), np.ones(5)], 1).ravel().astype(np.float32)
    g.set_parameters(mv, A, np.full(5, 0.2, np.float32))
    assert g.num_blocks() == WEAK_B
    return g


@pytest.fixture(scope="module")
def weak(hml, program):
    """the weak chain and the restatement's words for it, computed once for the cases below (the chain's geometry options change
    from case to case; nothing else of it does)"""
    g = weak_chain(hml)
    want = check(program, g)
    return g, want


def test_a_warm_up_of_one_block_leaves_chunks_stale(weak):
    """on the CPU: run from the uniform vector one block outside a chunk, the entry vector differs from the sequential
    recursion's in both directions, for every L used below"""
    g, want = weak
    case = pu.chain_case(g)
    e_rows = want["e"].view(np.float32).tolist()
    for L in (4, 64, 512):
        sub = dict(case, starts=case["starts"][:4 * L + 1])
        fwd, bwd = pu.stale_from_uniform(sub, e_rows[:4 * L], L, 1)
        assert fwd and bwd, L


@pytest.mark.parametrize("W", [1, 4, 64, 1024])
def test_geometry_is_invisible(weak, W):
    g, want = weak
    for L, rounds in itertools.product((4, 64, 512), (0, 1, 8)):
        g.set_option("posterior_W", W)
        g.set_option("posterior_L", L)
        g.set_option("posterior_rounds", rounds)
        t0 = time.perf_counter()
        check_results(g, want, (W, L, rounds))
        info = g.posterior_info()
        print("W %4d L %3d rounds %d: %s  %.0f ms" % (W, L, rounds, info, 1e3 * (time.perf_counter() - t0)))
        assert info["W"] == W and info["L"] == L and info["chunks"] == (WEAK_B + L - 1) // L and info["rounds"] <= rounds
        assert info["stale_fwd"] < info["chunks"] and info["stale_bwd"] < info["chunks"] and info["serial_chunks"] <= 2 * (info["chunks"] - 1)
        if W == 1:
            assert info["stale_fwd"] > 0 and info["stale_bwd"] > 0, (L, rounds)   # the repair ran, both ways ...
            if rounds == 0:
                assert info["serial_chunks"] > 0, L                                # ... and without rounds all of it on the single lane
        if info["stale_fwd"] + info["stale_bwd"] == 0 or rounds == 0:
            assert info["rounds"] == 0
        if info["stale_fwd"] + info["stale_bwd"] == 0:
            assert info["serial_chunks"] == 0


def test_geometry_rows_and_one_chunk(weak, program):
    g, want = weak
    # the rows too, under a geometry that repairs
    g.set_option("posterior_W", 1)
    g.set_option("posterior_L", 4)
    g.set_option("posterior_rounds", 1)
    check(program, g, what="rows")
    # one chunk: it starts from pi and from the last block and is right by construction
    g.set_option("posterior_L", 32768)
    check_results(g, want, "one chunk")
    info = g.posterior_info()
    assert info["chunks"] == 1 and info["stale_fwd"] == 0 and info["stale_bwd"] == 0 and info["serial_chunks"] == 0 and info["rounds"] == 0


@pytest.mark.parametrize("every_position", [False, True])
def test_twin_states(hml, program, every_position):
    """two states with identical emission parameters and sticky transitions forget their start very slowly
    (test_forward_repair_paths_on_twin_states of tests/test_gpu_parity.py)"""
    g = chain(hml, ol.trace(30000 if every_position else 300000, 3, 1), 3, sweeps=1, every_position=every_position)
    mv = np.array([-1.0, 0.04, 0.5, 0.04, 0.5, 0.04], np.float32)    # states 1 and 2 are twins
    A = np.array([[0.999, 0.0005, 0.0005], [0.0005, 0.9994, 0.0001], [0.0005, 0.0001, 0.9994]], np.float32)
    g.set_parameters(mv, A, np.array([0.2, 0.5, 0.3], np.float32))
    if not every_position:
        g.create_blocks(g.threshold())
    want = check(program, g)
    for W, L, rounds in [(1, 4, 0), (1, 64, 1), (4, 64, 8), (2, 512, 2), (1024, 4, 8)]:
        g.set_option("posterior_W", W)
        g.set_option("posterior_L", L)
        g.set_option("posterior_rounds", rounds)
        check_results(g, want, (W, L, rounds))


# ---------------------------------------------------------------------------------------------- memory, side effects
def test_a_call_keeps_no_device_memory_and_survives_failed_allocations(hml):
    g = chain(hml, ol.trace(5000, 3, 3), 3, every_position=True)
    g.set_option("posterior_W", 1)      # (stale chunks: the repair kernels run too)
    gc.collect()      # (chains that earlier tests dropped without closing go first: the totals below are this test's alone)
    before = hml.device_memory_live()
    calls = {"posterior": g.posterior, "posterior_rle": g.posterior_rle, "posterior_terms": g.posterior_terms}
    good = {}
    for name, call in calls.items():
        hml.debug_fail_allocation(10 ** 9)
        good[name] = call()
        n_alloc = hml.debug_fail_allocation(0)
        assert n_alloc >= 3 and hml.device_memory_live() == before, name
        for n in range(1, n_alloc + 1):
            hml.debug_fail_allocation(n)
            with pytest.raises(hml.HmlError) as e:
                call()
            hml.debug_fail_allocation(0)
            assert e.value.code == 2 and "out of memory" in str(e.value), (name, n)
            assert hml.device_memory_live() == before, (name, n)
        again = call()                # the next call succeeds, with the same answer
        flat = lambda r: [np.asarray(v).tobytes() for v in r]
        assert flat(again) == flat(good[name]) and hml.device_memory_live() == before, name


def test_calls_leave_the_chain_alone(hml):
    x = ol.trace(40000, 3, 13)

    def run(smooth):
        g = chain(hml, x, 3, seed=5, sweeps=0)
        g.iterate("F", 6, 2)
        if smooth:
            g.posterior(); g.posterior_rle(); g.posterior_terms(); g.posterior_info()
        g.iterate("F", 6, 2)
        if smooth:
            g.set_option("posterior_W", 1)
            g.posterior()
        g.iterate("M", 2, 1)
        g.sync()
        seg, cnt = g.marginals_rle()
        return g.states(), g.theta(), g.transitions(), seg, cnt, g.blocks()

    a, b = run(False), run(True)
    flat = lambda r: [np.asarray(v).tobytes() for part in r for v in (part if isinstance(part, tuple) else (part,))]
    assert flat(a) == flat(b)

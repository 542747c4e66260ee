"""Viterbi decode on the device (hml_viterbi ... hml_viterbi_info, include/hml.h) against the restatement for one host thread,
tests/fixtures/viterbi_ref_main.cpp over hammlet_amd/csrc/hml_viterbi_ref.h, which is fed the GPU's own block_stats(), blocks(),
theta() and transitions():
  (a) viterbi_scores() equals its tables bit for bit;
  (b) viterbi_states(), the run-length form and score_fixed equal its decode of those tables exactly.
Everything is an integer: there is no tolerance anywhere in this file."""
import gc
import itertools

import numpy as np
import pytest

from tests import hostile_inputs as hi
from tests import oracle_lib as ol
from tests import viterbi_util as vu

pytestmark = pytest.mark.gpu

DEFAULT_L = 64


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return vu.build_programs(tmp_path_factory.mktemp("viterbi_ref"), sanitized=False)["plain"]


def reference(program, g, self_trans=True):
    case = vu.chain_case(g, self_trans)
    want = vu.run_case(program, case)
    want["starts"] = case["starts"]
    return want


def check_decode(g, want, what=None):
    """(b): path per block, runs over positions and the score"""
    q = g.viterbi_states()
    assert np.array_equal(q, want["path"]), what
    run_len, run_state, (fixed, nats) = g.viterbi()
    want_len, want_state = vu.runs_of(want["path"], want["starts"])
    assert np.array_equal(run_len, want_len) and np.array_equal(run_state, want_state), what
    assert int(run_len.sum()) == g.T and np.all(run_state[1:] != run_state[:-1])
    assert fixed == want["score"] and nats == fixed / 2.0 ** 20, what
    return q


def check(program, g, self_trans=True, what=None):
    """(a) and (b)"""
    want = reference(program, g, self_trans)
    emit, trans, init = g.viterbi_scores()
    assert np.array_equal(init, want["init"]), what
    assert np.array_equal(trans, want["trans"]), what
    assert np.array_equal(emit, want["emit"]), what
    check_decode(g, want, what)
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
    check(program, g, what=T)
    info = g.viterbi_info()
    assert info["chunks"] == (g.num_blocks() + DEFAULT_L - 1) // DEFAULT_L and info["L"] == DEFAULT_L and info["W"] == 64


@pytest.mark.parametrize("B", [64 * DEFAULT_L - 1, 64 * DEFAULT_L, 64 * DEFAULT_L + 1, 70000])
def test_every_position_a_block(hml, program, B):
    g = chain(hml, ol.trace(B, 5, 4), 5, every_position=True)
    assert g.num_blocks() == B
    check(program, g, what=B)
    assert g.viterbi_info()["chunks"] == (B + DEFAULT_L - 1) // DEFAULT_L


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


def test_compat_context_decodes_to_the_same_tables(hml, program):
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
    for a, b in zip(c.viterbi_scores(), d.viterbi_scores()):
        assert np.array_equal(a, b)
    check_decode(d, want, "default")


def test_after_set_parameters_with_zeros_in_A_and_pi(hml, program):
    g = chain(hml, ol.trace(20000, 3, 9), 3, every_position=True)
    A = np.array([[0.5, 0.5, 0.0], [0.0, 0.5, 0.5], [1.0, 0.0, 0.0]], np.float32)
    pi = np.array([0.0, 1.0, 0.0], np.float32)
    g.set_parameters(np.array([-1.0, 0.05, 0.0, 0.05, 1.0, 0.05], np.float32), A, pi)
    want = check(program, g)
    low = -(2 ** 58)
    assert want["trans"][0, 2] == low and want["init"][0] == low and want["path"][0] == 1


def test_after_create_blocks_on_a_chain_that_never_iterated(hml, program):
    g = chain(hml, ol.trace(50000, 3, 11), 3, sweeps=0)
    with pytest.raises(hml.HmlError):
        g.viterbi()                       # no blocks yet
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


def test_geometry_is_invisible(hml, program):
    g = weak_chain(hml)
    want = check(program, g)
    # on the CPU first: a warm-up of one block from the zero vector does leave chunk 1 stale on this trace, for every L used
    emit, trans, init = [a.tolist() for a in g.viterbi_scores()]
    for L in (4, 64, 512):
        assert 1 in vu.stale_chunks_from_zero(emit[:2 * L], trans, init, L, 1), L
    for W, L, rounds in itertools.product((1, 4, 64, 1024), (4, 64, 512), (0, 1, 8)):
        g.set_option("viterbi_W", W)
        g.set_option("viterbi_L", L)
        g.set_option("viterbi_rounds", rounds)
        check_decode(g, want, (W, L, rounds))
        info = g.viterbi_info()
        print("W %4d L %3d rounds %d: %s" % (W, L, rounds, info))
        assert info["W"] == W and info["L"] == L and info["chunks"] == (WEAK_B + L - 1) // L and info["rounds"] <= rounds
        assert info["stale_chunks"] < info["chunks"] and info["serial_chunks"] <= info["chunks"] - 1   # (never chunk 0)
        if W == 1:
            assert info["stale_chunks"] > 0, (L, rounds)      # the repair ran ...
            if rounds == 0:
                assert info["serial_chunks"] > 0, L           # ... and without rounds all of it on the single lane
        if info["stale_chunks"] == 0 or rounds == 0:
            assert info["rounds"] == 0
        if info["stale_chunks"] == 0:
            assert info["serial_chunks"] == 0
    # one chunk: chunk 0 starts from init and is right by construction
    g.set_option("viterbi_W", 1)
    g.set_option("viterbi_L", 32768)
    check_decode(g, want, "one chunk")
    info = g.viterbi_info()
    assert info["chunks"] == 1 and info["stale_chunks"] == 0 and info["serial_chunks"] == 0 and info["rounds"] == 0


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
        g.set_option("viterbi_W", W)
        g.set_option("viterbi_L", L)
        g.set_option("viterbi_rounds", rounds)
        check_decode(g, want, (W, L, rounds))


# ---------------------------------------------------------------------------------------------- memory, side effects
def test_a_decode_keeps_no_device_memory_and_survives_failed_allocations(hml):
    g = chain(hml, ol.trace(5000, 3, 3), 3, every_position=True)
    g.set_option("viterbi_W", 1)      # (stale chunks: the repair kernels run too)
    gc.collect()      # (chains that earlier tests dropped without closing go first: the totals below are this test's alone)
    before = hml.device_memory_live()
    calls = {"viterbi": g.viterbi, "viterbi_states": g.viterbi_states, "viterbi_scores": g.viterbi_scores}
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
        again = call()                # the next decode succeeds, with the same answer
        flat = lambda r: [np.asarray(v).tolist() for v in (r if isinstance(r, tuple) else (r,))]
        assert flat(again) == flat(good[name]) and hml.device_memory_live() == before, name


def test_decodes_leave_the_chain_alone(hml):
    x = ol.trace(40000, 3, 13)

    def run(decode):
        g = chain(hml, x, 3, seed=5, sweeps=0)
        g.iterate("F", 6, 2)
        if decode:
            g.viterbi(); g.viterbi_states(); g.viterbi_scores(); g.viterbi_info()
        g.iterate("F", 6, 2)
        if decode:
            g.set_option("viterbi_W", 1)
            g.viterbi()
        g.iterate("M", 2, 1)
        g.sync()
        seg, cnt = g.marginals_rle()
        return g.states(), g.theta(), g.transitions(), seg, cnt, g.blocks()

    a, b = run(False), run(True)
    flat = lambda r: [np.asarray(v).tobytes() for part in r for v in (part if isinstance(part, tuple) else (part,))]
    assert flat(a) == flat(b)

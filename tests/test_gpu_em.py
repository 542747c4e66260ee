"""Expectation-maximisation on the device (hml_expected_counts, hml_em_step, hml_em_fit, include/hml.h) against the restatement
for one host thread, tests/fixtures/em_ref_main.cpp over hammlet_amd/csrc/hml_em_ref.h, which is fed the GPU's own
block_stats(), blocks(), theta() and transitions().  Every double is compared as its 64-bit word, every float as its 32-bit
word: there is no tolerance anywhere in this file."""
import gc
import numpy as np
import pytest

from tests import em_util as eu
from tests import hostile_inputs as hi
from tests import oracle_lib as ol
from tests import posterior_util as pu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return eu.build_programs(tmp_path_factory.mktemp("em_ref"), sanitized=False)["plain"]


def chain(hml, x, K, seed=3, sweeps=3, options=(), dims=None, self_trans=True, every_position=False):
    g = hml.Chain(device=0, seed=seed)
    for name, value in options:
        g.set_option(name, value)
    if dims:
        g.set_dimensions(*dims)
    g.load(x)
    if every_position:
        g.scale_weights(1e9)
    g.em_nig4 = g.autoprior(0.2, 0.9)
    g.set_model(K, g.em_nig4, self_trans=self_trans)
    g.sample_prior()
    if sweeps:
        g.iterate("F", sweeps, 0)
        g.sync()
    return g


def prior(g):
    return eu.prior_of(g.em_nig4, 0.5, 0.5, 0.5)     # (set_model's defaults for A's and pi's Dirichlet priors)


def check(program, g, self_trans=True, what=None):
    """expected_counts() equals the restatement's words"""
    want = eu.run_program(program, "estep", pu.chain_case(g, self_trans))
    got = eu.chain_counts_words(g.expected_counts())
    for key in eu.COUNT_KEYS + ("loglik",):
        assert np.array_equal(got[key], want[key]), (what, key)
    assert got["degenerate"] == want["degenerate"] and got["xi_degenerate"] == want["xi_degenerate"], what
    return want


@pytest.mark.parametrize("T", [2, 3, 16, 65])
def test_tiny_traces(hml, program, T):
    g = chain(hml, ol.trace(1000, 3, 2)[:T].copy(), 2, seed=12, sweeps=10)
    want = check(program, g, what=T)
    assert want["degenerate"] == 0 and want["xi_degenerate"] == 0
    n = g.expected_counts()
    assert abs(n["xi"].sum() - (g.num_blocks() - 1)) < 1e-9 and abs(n["occ"].sum() - T) < 1e-9


def test_one_block(hml, program):
    """a trace of one position is the context with B = 1: xi is all 0.0, and a fit still runs (a trace of two positions or more
    always has two blocks or more)"""
    g = hml.Chain(device=0, seed=12)
    g.load(np.array([0.3], np.float32))
    g.em_nig4 = np.array([2.0, 1.0, 0.0, 1.0], np.float32)      # (no automatic prior from one value)
    g.set_model(2, g.em_nig4)
    g.sample_prior()
    g.create_blocks(1.0)
    assert g.num_blocks() == 1
    want = check(program, g, what="B = 1")
    assert not want["xi"].any() and g.expected_counts()["first"].sum() == pytest.approx(1.0, abs=1e-15)
    case = pu.chain_case(g)
    want = eu.run_program(program, "fit", case, use_prior=True, prior=prior(g), max_steps=2)
    trace, steps, reason, kept = g.em_fit(2, use_prior=True)
    assert np.array_equal(pu.words(trace), want["trace"]) and (steps, reason, kept) == (want["steps"], want["reason"], want["kept"])
    assert np.array_equal(pu.words32(g.theta()), want["mean_var"]) and np.array_equal(pu.words32(g.transitions()[0]), want["A"])


@pytest.mark.parametrize("B", [64, 65, 66, 4096, 4097, 4098, 70000])
def test_every_position_a_block(hml, program, B):
    """the leaf-count boundaries of both trees (xi's has B - 1 leaves, the others' B) and three levels"""
    g = chain(hml, ol.trace(B, 5, 4), 5, every_position=True)
    assert g.num_blocks() == B
    want = check(program, g, what=B)
    assert want["degenerate"] == 0 and want["xi_degenerate"] == 0
    assert abs(g.expected_counts()["xi"].sum() - (B - 1)) < 1e-6 * B


@pytest.mark.parametrize("K", [2, 8, 9, 16, 17, 33, 64])
def test_numbers_of_states(hml, program, K):
    g = chain(hml, ol.trace(4100, min(K, 5), 7), K, every_position=True)
    assert g.num_blocks() == 4100
    check(program, g, what=K)


def test_blocks_of_many_positions(hml, program):
    g = chain(hml, ol.trace(30000, 5, 8), 5)
    assert g.num_blocks() < 30000
    check(program, g)
    n = g.expected_counts()
    assert abs(n["occ"].sum() - 30000) < 1e-6 * 30000 and np.all(n["stay"] <= n["occ"])


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


def test_compat_context(hml, program):
    g = chain(hml, ol.trace(20000, 3, 6), 3, options=[("compat", 1)], sweeps=5)
    g.create_blocks(g.threshold())
    check(program, g, what="compat")


def test_zeros_in_A_and_pi(hml, program):
    """(the diagonal of A stays positive, as the smoothing's test explains)"""
    g = chain(hml, ol.trace(20000, 3, 9), 3, every_position=True)
    A = np.array([[0.5, 0.5, 0.0], [0.0, 0.5, 0.5], [0.75, 0.0, 0.25]], np.float32)
    pi = np.array([0.0, 1.0, 0.0], np.float32)
    g.set_parameters(np.array([-1.0, 0.05, 0.0, 0.05, 1.0, 0.05], np.float32), A, pi)
    check(program, g)
    n = g.expected_counts()
    assert np.array_equal(n["xi"] == 0.0, A == 0.0) and n["first"].tolist() == [0.0, 1.0, 0.0]
    trace, steps, reason, kept = g.em_fit(2)
    A2, pi2 = g.transitions()
    assert steps >= 1 and np.array_equal(A2 == 0.0, A == 0.0) and np.array_equal(pi2, pi)


def test_a_block_no_path_reaches(hml, program):
    x = np.random.default_rng(2).normal(0, 0.3, 300).astype(np.float32)
    x[1:3] += 40.0
    g = chain(hml, x, 3, sweeps=1, every_position=True, self_trans=False)
    A = np.array([[0.5, 0.25, 0.25], [1.0, 0.0, 0.0], [0.25, 0.25, 0.5]], np.float32)
    mv = np.array([0.0, 1.0, 0.0, 1.0, 40.0, 1.0], np.float32)
    g.set_parameters(mv, A, np.array([0.0, 1.0, 0.0], np.float32))
    assert g.num_blocks() == 300
    want = check(program, g, self_trans=False)
    assert want["degenerate"] == 1 and want["xi_degenerate"] >= 1
    trace, steps, reason, kept = g.em_fit(5)
    assert (steps, reason, kept) == (0, hml.EM_DEGENERATE, 0) and len(trace) == 1 and trace[0] == -np.inf
    assert np.array_equal(g.theta(), mv) and np.array_equal(g.transitions()[0], A)


# ---------------------------------------------------------------------------------------------- geometry is invisible
def test_geometry_is_invisible(hml, program):
    """the decode's weakly separated trace: the words do not move under geometries of the smoothing pass that make the repair
    and the single lane run"""
    rng = np.random.default_rng(17)
    B = 20000
    st = np.cumsum(rng.random(B) < 0.01) % 5
    x = (0.5 * st + rng.normal(0, 1, B)).astype(np.float32)
    g = chain(hml, x, 5, sweeps=1, every_position=True)
    A = np.full((5, 5), 0.0025, np.float32)
    np.fill_diagonal(A, 0.99)
    mv = np.stack([0.5 * np.arange(5), np.ones(5)], 1).ravel().astype(np.float32)
    g.set_parameters(mv, A, np.full(5, 0.2, np.float32))
    assert g.num_blocks() == B
    check(program, g)
    first = eu.chain_counts_words(g.expected_counts())
    seen_repair = seen_serial = False
    for W, L, rounds in [(1, 4, 0), (1, 64, 1), (4, 512, 8), (1024, 64, 8), (1, 512, 2)]:
        g.set_option("posterior_W", W)
        g.set_option("posterior_L", L)
        g.set_option("posterior_rounds", rounds)
        got = eu.chain_counts_words(g.expected_counts())
        for key in eu.COUNT_KEYS + ("loglik",):
            assert np.array_equal(got[key], first[key]), (W, L, rounds, key)
        info = g.posterior_info()                 # the E-step's smoothing pass
        assert info["W"] == W and info["L"] == L
        seen_repair |= info["stale_fwd"] > 0 and info["stale_bwd"] > 0
        seen_serial |= info["serial_chunks"] > 0
    assert seen_repair and seen_serial


# ---------------------------------------------------------------------------------------------- the fit
@pytest.mark.parametrize("self_trans", [True, False])
def test_fit_reproduces_the_restatement(hml, program, self_trans):
    g = chain(hml, ol.trace(20000, 3, 21), 3, self_trans=self_trans)
    case = pu.chain_case(g, self_trans)
    mv, (A, pi) = g.theta(), g.transitions()
    for prior_on in (False, True):
        g.set_parameters(mv, A, pi)
        want = eu.run_program(program, "fit", case, use_prior=prior_on, prior=prior(g), max_steps=5)
        trace, steps, reason, kept = g.em_fit(5, use_prior=prior_on)
        assert np.array_equal(pu.words(trace), want["trace"]), prior_on
        assert (steps, reason, kept) == (want["steps"], want["reason"], want["kept"]), prior_on
        assert np.array_equal(pu.words32(g.theta()), want["mean_var"]), prior_on
        A2, pi2 = g.transitions()
        assert np.array_equal(pu.words32(A2), want["A"]) and np.array_equal(pu.words32(pi2), want["pi"]), prior_on
        assert steps >= 1 and trace[1] > trace[0]
        if not prior_on:
            assert pu.words([g.posterior()[1]])[0] == want["trace"][-1]       # log p(y | theta-hat) is the last trace entry
    g.iterate("F", 3, 0)                          # the chain's next sweeps run
    g.sync()
    assert np.isfinite(g.theta()).all()


def test_two_steps_equal_a_fit_of_two(hml, program):
    x = ol.trace(20000, 3, 22)
    a, b = chain(hml, x, 3), chain(hml, x, 3)
    obj = [a.em_step()[0], a.em_step()[0]]
    trace, steps, reason, kept = b.em_fit(2, rel_tol=-1.0)     # (a tolerance no step can meet: both M-steps run)
    assert steps == 2 and reason == hml.EM_MAX_STEPS
    assert np.array_equal(pu.words(obj), pu.words(trace[:2]))
    assert a.theta().tobytes() == b.theta().tobytes()
    assert [v.tobytes() for v in a.transitions()] == [v.tobytes() for v in b.transitions()]
    want = eu.run_program(program, "step", pu.chain_case(a), use_prior=True, prior=prior(a))
    o, kept = a.em_step(use_prior=True)
    assert pu.words([o])[0] == want["objective"][0] and kept == want["kept"]
    assert np.array_equal(pu.words32(a.theta()), want["mean_var"]) and np.array_equal(pu.words32(a.transitions()[0]), want["A"])


# ---------------------------------------------------------------------------------------------- memory, side effects
def test_calls_keep_no_device_memory_and_survive_failed_allocations(hml):
    g = chain(hml, ol.trace(5000, 3, 3), 3, every_position=True)
    g.set_option("posterior_W", 1)      # (stale chunks: the repair kernels run too)
    mv, (A, pi) = g.theta(), g.transitions()
    gc.collect()      # (chains that earlier tests dropped without closing go first: the totals below are this test's alone)
    before = hml.device_memory_live()
    flat = lambda r: [np.asarray(v).tobytes() for v in (r.values() if isinstance(r, dict) else r)]
    for name, call in {"expected_counts": g.expected_counts, "em_fit": lambda: g.em_fit(1)}.items():
        g.set_parameters(mv, A, pi)
        hml.debug_fail_allocation(10 ** 9)
        good = call()
        n_alloc = hml.debug_fail_allocation(0)
        assert n_alloc >= 5 and hml.device_memory_live() == before, name
        for n in range(1, n_alloc + 1):
            g.set_parameters(mv, A, pi)
            hml.debug_fail_allocation(n)
            with pytest.raises(hml.HmlError) as e:
                call()
            hml.debug_fail_allocation(0)
            assert e.value.code == 2 and "out of memory" in str(e.value), (name, n)
            assert hml.device_memory_live() == before, (name, n)
        g.set_parameters(mv, A, pi)
        assert flat(call()) == flat(good) and hml.device_memory_live() == before, name


def test_expected_counts_leave_the_chain_alone(hml):
    x = ol.trace(40000, 3, 13)

    def run(count):
        g = chain(hml, x, 3, seed=5, sweeps=0)
        g.iterate("F", 6, 2)
        if count:
            g.expected_counts()
        g.iterate("F", 6, 2)
        if count:
            g.set_option("posterior_W", 1)
            g.expected_counts()
        g.iterate("M", 2, 1)
        g.sync()
        seg, cnt = g.marginals_rle()
        return g.states(), g.theta(), g.transitions(), seg, cnt, g.blocks()

    a, b = run(False), run(True)
    flat = lambda r: [np.asarray(v).tobytes() for part in r for v in (part if isinstance(part, tuple) else (part,))]
    assert flat(a) == flat(b)

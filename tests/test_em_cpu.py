"""Expectation-maximisation restated for one host thread (hammlet_amd/csrc/hml_em_ref.h) as a stand-alone program,
tests/fixtures/em_ref_main.cpp: built with g++ -Wall -Werror -ffp-contract=off, and a second time with the address and
undefined-behaviour sanitizers (nothing is loaded into Python for this), against the restatement in Python floats of
tests/em_util.py.  Both sides derive every word from the same floats by the same IEEE operations in the same order, so (a)
compares words.

(b) compares the Python restatement - and, on the same cases, the program's words with it - with an enumeration of all K^B
paths: xi, first, occ and sx within 1e-12 relative, the bound the smoothing's test derives (tests/test_posterior_cpu.py).

(d) EM behaves as EM: the objective may fall only by the rounding of the float tables.  FALL_MEASURED is the worst relative
fall of a step of the Python restatement over the cases and seeds of this file (printed by the test); the cap is four times
that, because the fall is rounding noise and varies with the seed.  It was measured on the restatement, never on the device."""
import math

import numpy as np
import pytest

from tests import em_util as eu
from tests import posterior_util as pu

PRIOR = eu.prior_of([2.0, 1.0, 0.25, 0.5], 1.5, 3.0, 1.25)


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    return eu.build_programs(tmp_path_factory.mktemp("em_ref"))


# ---------------------------------------------------------------------------------------------- (a) word for word
def check_case(programs, case, what):
    want = eu.estep(case)
    fits = {}
    for prior_on in (False, True):
        fits[prior_on] = eu.fit(case, 5, 0.0, prior_on, PRIOR)
    for name, exe in programs.items():
        w = (what, name)
        eu.same_counts(eu.run_program(exe, "estep", case), want, w)
        for prior_on in (False, True):
            got = eu.run_program(exe, "step", case, use_prior=prior_on, prior=PRIOR)
            after, kept = eu.mstep(case, want, prior_on, PRIOR)
            assert got["objective"][0] == eu.words([eu.objective(case, want["loglik"], prior_on, PRIOR)])[0], w
            assert got["kept"] == kept, w
            eu.same_parameters(got, after, w + (prior_on,))
            final, trace, steps, reason, kept = fits[prior_on]
            got = eu.run_program(exe, "fit", case, use_prior=prior_on, prior=PRIOR, max_steps=5)
            assert np.array_equal(got["trace"], eu.words(trace)), w + (prior_on,)
            assert (got["steps"], got["reason"], got["kept"]) == (steps, reason, kept), w
            eu.same_parameters(got, final, w + (prior_on, "fit"))
    return want, fits


@pytest.mark.parametrize("B", [1, 2, 64, 65, 66, 200])
@pytest.mark.parametrize("K", [2, 3, 5])
def test_every_word_equals_the_python_restatement(programs, K, B):
    rng = np.random.default_rng(1000 * K + B)
    want, fits = check_case(programs, pu.random_case(rng, K, B), (K, B))
    assert want["degenerate"] == 0 and want["xi_degenerate"] == 0
    if B == 1:
        assert all(v == 0.0 for row in want["xi"] for v in row)


def test_two_dimensions_two_parameters_word_for_word(programs):
    rng = np.random.default_rng(7)
    for B in (65, 130):
        check_case(programs, pu.random_case(rng, 4, B, D=2, P=2), ("D2", B))


def test_self_transitions_off_word_for_word(programs):
    rng = np.random.default_rng(8)
    for B in (64, 129):
        check_case(programs, pu.random_case(rng, 3, B, self_trans=False), ("off", B))


def test_streaming_tree_equals_the_list_tree(programs):
    """B = 4097 + 1: xi's tree has 4097 leaves and three levels, the others' 4098"""
    rng = np.random.default_rng(9)
    case = pu.random_case(rng, 2, 4098, max_len=2)
    want = eu.estep(case)
    eu.same_counts(eu.run_program(programs["plain"], "estep", case), want, 4098)


# ---------------------------------------------------------------------------------------------- (b) all paths
@pytest.mark.parametrize("seed", range(8))
def test_against_all_paths(programs, seed):
    rng = np.random.default_rng(2000 + seed)
    checked = 0
    while checked < 5:
        K, B = int(rng.integers(2, 4)), int(rng.integers(1, 8))
        case = pu.random_case(rng, K, B)
        if rng.random() < 0.3:
            A = case["A"].copy()
            i = int(rng.integers(K))
            A[i, (i + 1 + int(rng.integers(K - 1))) % K] = 0.0
            case["A"] = (A / A.sum(1, keepdims=True)).astype(np.float32)
        want = eu.enumerate_counts(case)
        got = eu.estep(case)
        if want is None:
            assert got["degenerate"] > 0
            continue
        assert got["degenerate"] == 0 and got["xi_degenerate"] == 0

        def near(a, b):
            return a == 0.0 if b == 0.0 else abs(a - b) <= 1e-12 * abs(b)
        for i in range(K):
            assert near(got["first"][i], want["first"][i]) and near(got["occ"][i], want["occ"][i]), (K, B, i)
            for j in range(K):
                assert near(got["xi"][i][j], want["xi"][i][j]), (K, B, i, j)
            for d in range(case["D"]):
                assert near(got["sx"][i][d], want["sx"][i][d]), (K, B, i, d)
        eu.same_counts(eu.run_program(programs["plain"], "estep", case), got, (K, B))      # the header's words are these
        checked += 1


# ---------------------------------------------------------------------------------------------- (c) identities
def test_identities():
    rng = np.random.default_rng(31)
    for K, B, D, P in [(2, 70, 1, None), (3, 130, 1, None), (4, 40, 2, 2), (5, 65, 1, None)]:
        case = pu.random_case(rng, K, B, D=D, P=P)
        n = eu.estep(case)
        T = int(case["starts"][-1])
        for j in range(K):
            col = math.fsum(n["xi"][i][j] for i in range(K))
            gam = math.fsum(n["gamma"][b][j] for b in range(1, B))
            assert abs(col - gam) <= 1e-9 * max(1.0, gam), (K, B, j)
        assert abs(math.fsum(n["occ"]) - T) <= 1e-9 * T
        assert abs(math.fsum(n["first"]) - 1.0) <= 1e-12
        for j in range(K):
            assert abs((n["occ"][j] - n["stay"][j]) - math.fsum(n["gamma"][b][j] for b in range(B))) <= 1e-9 * B


def test_a_fixed_point_is_returned(programs):
    """two states with the same emission parameters, A = 1/2 throughout and pi = (1/2, 1/2): every xi_b is 1/4 exactly, every
    gamma 1/2, and the M-step gives A and pi back"""
    rng = np.random.default_rng(5)
    case = pu.random_case(rng, 2, 9, self_trans=False)
    case["mean_var"] = np.array([0.5, 1.5, 0.5, 1.5], np.float32)
    case["A"] = np.full((2, 2), 0.5, np.float32)
    case["pi"] = np.full(2, 0.5, np.float32)
    n = eu.estep(case)
    after, kept = eu.mstep(case, n)
    assert kept == 0 and n["xi"] == [[2.0, 2.0], [2.0, 2.0]] and n["first"] == [0.5, 0.5]
    assert np.array_equal(after["A"], case["A"]) and np.array_equal(after["pi"], case["pi"])
    eu.same_parameters(eu.run_program(programs["sanitized"], "step", case), after)


# ---------------------------------------------------------------------------------------------- (d) EM behaves as EM
LEVELS, SIGMA, SWITCH_B = (-1.0, 0.0, 1.2), 0.4, 300
FALL_MEASURED = 9.02e-7      # worst relative fall of a step over the cases below: 9.014e-07 (K = 3, prior on, seed 3), rounded up
FALL_CAP = 4 * FALL_MEASURED
SWITCH_CASES = [(3, True, False), (3, True, True), (4, False, False)]     # K, self-transitions, prior
SWITCH_SEEDS = (1, 2, 3)


def switching_case(seed, K, self_trans):
    """a Markov-switching trace: levels -1, 0, 1.2, sigma 0.4, 300 blocks of 1 ... 39 positions; deliberately poor start"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 40, SWITCH_B)
    state = np.zeros(SWITCH_B, np.int64)
    for b in range(1, SWITCH_B):
        state[b] = state[b - 1] if rng.random() < 0.8 else rng.integers(3)
    sx, sq = np.empty(SWITCH_B, np.float32), np.empty(SWITCH_B, np.float32)
    for b in range(SWITCH_B):
        x = rng.normal(LEVELS[state[b]], SIGMA, lens[b]).astype(np.float32)
        sx[b], sq[b] = x.sum(dtype=np.float32), (x * x).sum(dtype=np.float32)
    mean = np.linspace(-0.5, 0.8, K).astype(np.float32)
    mv = np.stack([mean, np.ones(K, np.float32)], 1).ravel()
    A = np.full((K, K), 0.2 / (K - 1), np.float32)
    np.fill_diagonal(A, 0.8)
    return pu.make_case(K, np.concatenate([[0], np.cumsum(lens)]), sx, sq, mv, A, np.full(K, 1.0 / K, np.float32), self_trans=self_trans)


@pytest.mark.parametrize("K,self_trans,prior_on", SWITCH_CASES)
def test_the_objective_rises(K, self_trans, prior_on):
    worst = 0.0
    for seed in SWITCH_SEEDS:
        case = switching_case(seed, K, self_trans)
        trace = []
        for _ in range(25):
            n = eu.estep(case)
            assert n["degenerate"] + n["xi_degenerate"] == 0
            trace.append(eu.objective(case, n["loglik"], prior_on, PRIOR))
            case, kept = eu.mstep(case, n, prior_on, PRIOR)
            assert kept == 0
        trace.append(eu.objective(case, eu.estep(case)["loglik"], prior_on, PRIOR))
        falls = [(a - b) / abs(a) for a, b in zip(trace, trace[1:]) if b < a]
        worst = max([worst] + falls)
        print("K %d self %d prior %d seed %d: %.3f -> %.3f, worst relative fall %.3g" % (K, self_trans, prior_on, seed, trace[0], trace[-1], max(falls + [0.0])))
        assert all(math.isfinite(v) for v in trace)
        assert trace[-1] - trace[0] > 100.0, (seed, trace[0], trace[-1])          # hundreds of nats at the least, from the poor start
        assert all(f <= FALL_CAP for f in falls), (seed, max(falls))
        assert trace[1] > trace[0] and trace[2] > trace[1]
    assert worst <= FALL_MEASURED


def test_the_program_climbs_the_same_trace(programs):
    """25 steps of the program's fit on a switching case, with the prior on: the restatement's trace and parameters, word for word"""
    case = switching_case(SWITCH_SEEDS[0], 3, True)
    final, trace, steps, reason, kept = eu.fit(case, 25, -1.0, True, PRIOR)        # (a tolerance no step meets: all 25 run)
    assert steps == 25 and reason == eu.MAX_STEPS and trace[-1] - trace[0] > 100.0
    for name, exe in programs.items():
        got = eu.run_program(exe, "fit", case, use_prior=True, prior=PRIOR, max_steps=25, rel_tol=-1.0)
        assert np.array_equal(got["trace"], eu.words(trace)), name
        assert (got["steps"], got["reason"], got["kept"]) == (steps, reason, kept), name
        eu.same_parameters(got, final, name)


# ---------------------------------------------------------------------------------------------- (e) empty and hostile cases
def test_a_state_no_block_supports_keeps_its_parameters(programs):
    """state 2's level lies hundreds of sigma from every block: its e underflows to 0 everywhere, occ[2] = 0 exactly.  With the
    prior on (every a > 1) the emission parameter alone is kept; under maximum likelihood its row of A has no support either"""
    rng = np.random.default_rng(12)
    case = pu.random_case(rng, 3, 70, self_trans=False)
    mv = case["mean_var"].copy()
    mv[4], mv[5] = 500.0, 0.25
    case["mean_var"] = mv
    n = eu.estep(case)
    assert n["occ"][2] == 0.0 and n["first"][2] == 0.0 and all(v == 0.0 for v in n["xi"][2])
    after, kept = eu.mstep(case, n, True, PRIOR)
    assert kept == 1 and after["mean_var"][4] == np.float32(500.0) and after["mean_var"][5] == np.float32(0.25)
    assert after["mean_var"][0] != case["mean_var"][0]
    eu.same_parameters(eu.run_program(programs["sanitized"], "step", case, use_prior=True, prior=PRIOR), after)
    after, kept = eu.mstep(case, n, False)
    assert kept == 2 and np.array_equal(after["A"][2], case["A"][2]) and after["mean_var"][4] == np.float32(500.0)
    got = eu.run_program(programs["sanitized"], "step", case)
    assert got["kept"] == 2
    eu.same_parameters(got, after)


def test_zeros_in_A_and_pi_stay_zero_under_maximum_likelihood(programs):
    rng = np.random.default_rng(6)
    case = pu.random_case(rng, 3, 50)
    case["A"] = np.array([[0.5, 0.5, 0.0], [0.0, 0.5, 0.5], [0.75, 0.0, 0.25]], np.float32)
    case["pi"] = np.array([0.0, 1.0, 0.0], np.float32)
    final, trace, steps, reason, kept = eu.fit(case, 3)
    assert steps >= 1 and kept == 0
    assert np.array_equal(final["A"] == 0.0, case["A"] == 0.0) and np.array_equal(final["pi"], case["pi"])
    got = eu.run_program(programs["sanitized"], "fit", case, max_steps=3)
    eu.same_parameters(got, final)
    assert np.array_equal(got["trace"], eu.words(trace))


def test_an_unreachable_block_ends_the_fit(programs):
    """the smoothing test's case: pi = (0, 1, 0), state 1 leads to state 0 alone, block 1 lies 40 sigma from state 0's level"""
    starts = np.arange(5)
    x = np.array([0.0, 40.0, 40.0, 0.0], np.float32)
    case = pu.make_case(3, starts, x, x * x, np.array([0.0, 1.0, 0.0, 1.0, 40.0, 1.0], np.float32),
                        np.array([[0.5, 0.25, 0.25], [1.0, 0.0, 0.0], [0.25, 0.25, 0.5]], np.float32), np.array([0.0, 1.0, 0.0], np.float32), self_trans=False)
    n = eu.estep(case)
    assert n["degenerate"] == 1 and n["xi_degenerate"] >= 1
    assert not any(math.isnan(v) for row in n["xi"] for v in row)
    final, trace, steps, reason, kept = eu.fit(case, 5)
    assert (steps, reason, kept) == (0, eu.DEGENERATE, 0) and len(trace) == 1 and trace[0] == -math.inf
    for name, exe in programs.items():
        eu.same_counts(eu.run_program(exe, "estep", case), n, name)
        got = eu.run_program(exe, "fit", case, max_steps=5)
        assert (got["steps"], got["reason"], got["kept"]) == (0, eu.DEGENERATE, 0)
        eu.same_parameters(got, case)

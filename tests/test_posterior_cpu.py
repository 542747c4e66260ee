"""The smoothing restatement for one host thread (hammlet_amd/csrc/hml_posterior_ref.h) as a stand-alone program,
tests/fixtures/posterior_ref_main.cpp: built with g++ -Wall -Werror -ffp-contract=off, and a second time with the address and
undefined-behaviour sanitizers (nothing is loaded into Python for this), against the restatement in Python floats of
tests/posterior_util.py.  Both sides derive every word from the same floats by the same IEEE operations in the same order, so
everything is compared for equality of words.

The Python restatement in turn is compared with an enumeration of all K^B paths (weights in double, sums by math.fsum).
Tolerance there: every sum of the recursions is over non-negative terms, so the error of a posterior or of c_0 ... c_{B-1} is
componentwise at most about 2 B (K + 3) units of 2^-53 - about 1e-14 for K <= 3, B <= 7; the bound 1e-12 leaves a factor of 100."""
import math

import numpy as np
import pytest

from tests import posterior_util as pu
from tests.posterior_util import random_case


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    return pu.build_programs(tmp_path_factory.mktemp("posterior_ref"))


def same_words(got, want, what):
    got, want = np.asarray(got), pu.words(np.array(want, np.float64))
    assert got.shape == want.shape or got.size == want.size, what
    assert np.array_equal(got.ravel(), want), what


def check(programs, case, what):
    """both builds against the Python restatement: e, m, alpha, c, beta, gamma, log-likelihood, runs"""
    e, m = pu.tables(case)
    want = pu.smooth(case, e, m)
    for name, exe in programs.items():
        got = pu.run_case(exe, case)
        w = (what, name)
        assert np.array_equal(got["e"].ravel(), pu.words32(np.array(e, np.float32))), w
        assert np.array_equal(got["m"], pu.words32(np.array(m, np.float32))), w
        for key in ("alpha", "c", "beta", "gamma", "run_conf"):
            same_words(got[key], want[key], w + (key,))
        same_words(got["loglik"], [want["loglik"]], w)
        assert got["degenerate"] == want["degenerate"], w
        assert got["state"].tolist() == want["state"] and got["run_len"].tolist() == want["run_len"] and got["run_state"].tolist() == want["run_state"], w
    return e, m, want


@pytest.mark.parametrize("K,B,D,P,self_trans", [(2, 1, 1, None, True), (2, 2, 1, None, True), (3, 7, 1, None, True), (5, 40, 1, None, True),
                                                (5, 40, 1, None, False), (4, 33, 2, 2, True), (20, 9, 1, None, True),
                                                (2, 64, 1, None, True), (2, 65, 1, None, True), (2, 4097, 1, None, True)])
def test_every_word_equals_the_python_restatement(programs, K, B, D, P, self_trans):
    rng = np.random.default_rng(100 * K + B)
    e, m, want = check(programs, random_case(rng, K, B, D=D, P=P, self_trans=self_trans, max_len=2 if B > 1000 else 5), (K, B, D))
    assert want["degenerate"] == 0 and math.isfinite(want["loglik"])
    assert sum(want["run_len"]) > 0 and all(a != b for a, b in zip(want["run_state"], want["run_state"][1:]))
    for row in want["gamma"]:
        assert abs(sum(row) - 1.0) < 1e-14


def test_tree_levels():
    """the order of the sum is the definition's: 64 consecutive values per value of the next level"""
    v = [0.1 * (i % 7) - 1e-3 * i for i in range(4097)]
    level1 = []
    for i in range(0, 4097, 64):
        s = v[i]
        for x in v[i + 1:i + 64]:
            s = s + x
        level1.append(s)
    assert len(level1) == 65
    s = level1[0]
    for x in level1[1:64]:
        s = s + x
    assert pu.tree_sum(v) == s + level1[64] and pu.tree_sum(v[:64]) == pu.tree_sum([pu.tree_sum(v[:64])]) and pu.tree_sum([2.5]) == 2.5


def test_zeros_in_A_and_pi(programs):
    rng = np.random.default_rng(6)
    case = random_case(rng, 3, 50)
    case["A"] = np.array([[0.5, 0.5, 0.0], [0.0, 0.5, 0.5], [0.75, 0.0, 0.25]], np.float32)   # (the diagonal stays positive: see below)
    case["pi"] = np.array([0.0, 1.0, 0.0], np.float32)
    e, m, want = check(programs, case, "zeros")
    assert want["degenerate"] == 0 and math.isfinite(want["loglik"])
    assert want["gamma"][0] == [0.0, 1.0, 0.0] and want["gamma"][1][0] == 0.0 and want["state"][0] == 1


def test_a_block_no_path_reaches_is_degenerate(programs):
    """pi puts everything on state 1, A sends state 1 to state 0 alone, and block 1 lies 40 sigma from state 0's level: e_1(0)
    underflows to 0 and c_1 = 0.  One degenerate block, log p = -inf, and no not-a-number in gamma.  (Self-transitions off: with
    them a block of one position in a state with A_jj = 0 has E = 0 x -inf, not a number, a different matter.)"""
    starts = np.arange(5)
    x = np.array([0.0, 40.0, 40.0, 0.0], np.float32)
    case = pu.make_case(3, starts, x, x * x, np.array([0.0, 1.0, 0.0, 1.0, 40.0, 1.0], np.float32),
                        np.array([[0.5, 0.25, 0.25], [1.0, 0.0, 0.0], [0.25, 0.25, 0.5]], np.float32), np.array([0.0, 1.0, 0.0], np.float32), self_trans=False)
    e, m, want = check(programs, case, "degenerate")
    assert e[1][0] == 0.0 and want["c"][1] == 0.0
    assert want["degenerate"] == 1 and want["loglik"] == -math.inf
    assert not np.isnan(np.array(want["gamma"])).any() and not np.isnan(np.array(want["beta"])).any()
    assert want["alpha"][1] == [1.0 / 3] * 3 and want["gamma"][0] == want["alpha"][0] == [0.0, 1.0, 0.0]


@pytest.mark.parametrize("seed", range(12))
def test_against_all_paths(seed):
    rng = np.random.default_rng(1000 + seed)
    checked = 0
    while checked < 6:
        K, B = int(rng.integers(2, 4)), int(rng.integers(1, 8))
        case = random_case(rng, K, B)
        if rng.random() < 0.3:                      # a zero off the diagonal of A, and sometimes in pi
            A = case["A"].copy()
            i = int(rng.integers(K))
            A[i, (i + 1 + int(rng.integers(K - 1))) % K] = 0.0
            case["A"] = (A / A.sum(1, keepdims=True)).astype(np.float32)
            if rng.random() < 0.5:
                pi = case["pi"].copy()
                pi[int(rng.integers(K))] = 0.0
                case["pi"] = (pi / pi.sum()).astype(np.float32)
        e, m = pu.tables(case)
        got = pu.smooth(case, e, m)
        gamma, loglik = pu.enumerate_paths(case, e, m)
        if gamma is None:                           # the zeros left no path a weight: the recursion must say so, and another case is drawn
            assert got["degenerate"] > 0 and got["loglik"] == -math.inf, (K, B)
            continue
        assert got["degenerate"] == 0
        for b in range(B):
            for s in range(K):
                if gamma[b][s] == 0.0:
                    assert got["gamma"][b][s] == 0.0, (K, B, b, s)
                else:
                    assert abs(got["gamma"][b][s] - gamma[b][s]) <= 1e-12 * gamma[b][s], (K, B, b, s)
        assert abs(got["loglik"] - loglik) <= 1e-12 * max(1.0, abs(loglik)), (K, B)
        checked += 1
    assert checked == 6

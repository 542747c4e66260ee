"""Path sampling under fixed parameters restated for one host thread (hammlet_amd/csrc/hml_sample_ref.h) as a stand-alone
program, tests/fixtures/sample_ref_main.cpp: built with g++ -Wall -Werror -ffp-contract=off, and a second time with the
address and undefined-behaviour sanitizers (nothing is loaded into Python for this), against the restatement of
tests/sample_util.py.  Both sides derive every word from the same floats by the same IEEE operations in the same order, so
(a) compares integers: paths, segments, scores, change and state counts, region counts and the degenerate count.

(b) The sampler samples the posterior: the count of every one of the K^B paths among R = 200 000 draws of the restatement
against R p from the enumeration, cells with R p < 5 pooled into one.  The bound is Bernstein's inequality at delta = 1e-12 per
cell, |count - R p| <= L/3 + sqrt(L^2/9 + 2 v L) with v = R p (1 - p) and L = ln(2 / delta): it is derived, not measured, and
holds for skewed cells, which a fixed number of standard deviations does not.  With at most 2188 cells, three seeds and four
cases the chance that a correct sampler fails is below 3e-8.  The seeds are 1, 2 and 3."""
import numpy as np
import pytest

from tests import pairs_util as pr
from tests import posterior_util as pu
from tests import sample_util as su

R_STAT = 200000


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("sample_ref")
    return su.build_programs(d), str(d)


# ---------------------------------------------------------------------------------------------- (a) word for word
def check_case(programs, case, what, first=0, count=9, seed=5, degenerate=False):
    exes, d = programs
    K = case["K"]
    rng = np.random.default_rng(11)
    start, end = pr.edge_regions(case["starts"], rng, n_random=3)
    H = 3
    want = su.restate(case, first, count, seed, start, end, H)
    for name, exe in exes.items():
        got = su.run_program(exe, case, first, count, seed, start, end, H, paths_file=d + "/paths_" + name)
        assert np.array_equal(got["alpha"], want["alpha"]), (what, name)
        assert np.array_equal(got["paths"], want["paths"]), (what, name)
        su.same(got, want, su.COUNT_KEYS + su.REGION_KEYS + ("viterbi_score",), (what, name))
    su.invariants(want, K, count, want["viterbi_score"], *(() if degenerate else (case["A"], case["pi"])))
    assert np.all(want["hist"].sum(1) == count) and np.all(want["whole_state"].sum(1) == want["hist"][:, 0])
    return want


@pytest.mark.parametrize("B", [1, 2, 64, 65, 200])
@pytest.mark.parametrize("K", [2, 3, 5])
def test_every_word_equals_the_python_restatement(programs, K, B):
    rng = np.random.default_rng(1000 * K + B)
    want = check_case(programs, su.random_case(rng, K, B), (K, B))
    assert want["sample_degenerate"] == 0
    if B == 1:
        assert np.all(want["segments"] == 1) and want["change_count"][0] == 0


def test_two_dimensions_two_parameters_word_for_word(programs):
    rng = np.random.default_rng(7)
    for B in (65, 130):
        check_case(programs, su.random_case(rng, 4, B, D=2, P=2), ("D2", B))


def test_self_transitions_off_word_for_word(programs):
    rng = np.random.default_rng(8)
    for B in (64, 129):
        check_case(programs, su.random_case(rng, 3, B, self_trans=False), ("off", B))


def zeros_case(rng, B):
    case = su.random_case(rng, 3, B)
    case["A"] = np.array([[0.5, 0.5, 0.0], [0.0, 0.5, 0.5], [0.75, 0.0, 0.25]], np.float32)
    case["pi"] = np.array([0.0, 1.0, 0.0], np.float32)
    return case


def test_zeros_in_A_and_pi(programs):
    rng = np.random.default_rng(9)
    want = check_case(programs, zeros_case(rng, 70), "zeros", count=40)
    assert want["sample_degenerate"] == 0 and np.all(want["paths"][:, 0] == 1)


def unreachable_case():
    """pi = (0, 1, 0), state 1 leads to state 0 alone, and block 1 lies 40 sigma from state 0's level: c_1 = 0 (the
    smoothing's tests have this block)"""
    x = np.random.default_rng(2).normal(0, 0.3, 30).astype(np.float32)
    x[1:3] += 40.0
    A = np.array([[0.5, 0.25, 0.25], [1.0, 0.0, 0.0], [0.25, 0.25, 0.5]], np.float32)
    return pu.make_case(3, np.arange(31), x, x * x, np.array([0.0, 1.0, 0.0, 1.0, 40.0, 1.0], np.float32), A, np.array([0.0, 1.0, 0.0], np.float32),
                        self_trans=False)


def test_a_block_no_path_reaches(programs):
    """alpha_1 is the uniform restart; given q_1 = 2, which nothing but the restart allows, block 0 has w = alpha_0 A[., 2] =
    (0, 1, 0) x (0.25, 0, 0.5) = 0: degenerate for that draw, which then takes q_0 from alpha_0"""
    want = check_case(programs, unreachable_case(), "unreachable", count=64, degenerate=True)
    q = want["paths"]
    assert want["sample_degenerate"] == int((q[:, 1] == 2).sum()) > 0
    assert np.all(q[:, 0] == 1)


def test_windows_are_slices(programs):
    exes, d = programs
    case = su.random_case(np.random.default_rng(21), 3, 65)
    whole = su.run_program(exes["plain"], case, 0, 16, 3, paths_file=d + "/w16")
    part = su.run_program(exes["plain"], case, 5, 4, 3, paths_file=d + "/w4")
    assert np.array_equal(part["paths"], whole["paths"][5:9])
    assert np.array_equal(part["segments"], whole["segments"][5:9]) and np.array_equal(part["score_fixed"], whole["score_fixed"][5:9])
    far = su.restate(case, 2 ** 48 - 4, 4, 3)
    got = su.run_program(exes["sanitized"], case, 2 ** 48 - 4, 4, 3, paths_file=d + "/wfar")
    assert np.array_equal(got["paths"], far["paths"])
    other = su.run_program(exes["plain"], case, 0, 16, 4, paths_file=d + "/wseed")
    assert not np.array_equal(other["paths"], whole["paths"])


def test_the_categorical_rule_at_both_ends_of_u(programs):
    exes, _ = programs
    top = 1.0 - 2.0 ** -53                    # the largest uniform
    tiny = 5e-324                             # the smallest positive double
    cases = [([0.0, 0.25, 0.0, 0.75, 0.0], 0.0, 1), ([0.0, 0.25, 0.0, 0.75, 0.0], top, 3), ([0.5, 0.5], 0.5, 1), ([0.5, 0.5], 0.5 - 2.0 ** -54, 0),
             ([1.0, 0.0, 0.0], top, 0), ([0.0, 0.0, 1.0], 0.0, 2),
             ([3.0, 0.0], top, 0),
             # t = u S rounds up to S = c_{K-1} (among normal numbers it cannot: S 2^-53 is more than half a unit in the last
             # place of S unless S is a power of two, and then t is exact): the largest state of positive weight, not the zero behind
             ([0.0, tiny, 0.0], top, 1), ([tiny, tiny, 0.0, 0.0], top, 1), ([tiny, 0.0], 0.0, 0)]
    for w, u, want in cases:
        state, _ = su.pick(np.array([w], np.float64), np.array([u]))
        assert int(state[0]) == want, (w, u)
        for exe in exes.values():
            assert su.run_pick(exe, w, u) == want, (w, u)
    assert not (top * tiny < tiny) and not (top * (2 * tiny) < 2 * tiny)      # the rounding cases are such


def test_uniforms():
    """in [0, 1), on the 2^-53 grid, distinct per (seed, draw, block), and both halves of a Philox block are used"""
    r = np.arange(1000, dtype=np.uint64)
    u0, u1, u2 = su.uniforms(9, r, 0), su.uniforms(9, r, 1), su.uniforms(9, r, 2)
    for u in (u0, u1, u2):
        assert np.all((u >= 0.0) & (u < 1.0)) and np.all(u * 2.0 ** 53 == np.floor(u * 2.0 ** 53))
        assert 0.45 < u.mean() < 0.55
    assert not np.array_equal(u0, u1) and not np.array_equal(u0, u2) and not np.array_equal(u0, su.uniforms(10, r, 0))
    assert np.array_equal(su.uniforms(9, r + np.uint64(2 ** 32), 0)[:5] == u0[:5], np.zeros(5, bool))     # the high word of the draw counts
    # a known answer of Philox4x32-10 (Random123's kat_vectors): counter and key all zero
    o = su.philox4x32_10(0, 0, 0, 0, 0, 0)
    assert [int(v) for v in o] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]


# ---------------------------------------------------------------------------------------------- (b) the posterior
def stat_cases():
    rng = np.random.default_rng(77)
    cases = [("K2B7", su.random_case(rng, 2, 7)), ("K3B5", su.random_case(rng, 3, 5)), ("K3B7", su.random_case(rng, 3, 7)), ("zeros", zeros_case(rng, 6))]
    return cases


@pytest.fixture(scope="module")
def probabilities():
    return {name: (case, su.path_probabilities(case)) for name, case in stat_cases()}


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("name", ["K2B7", "K3B5", "K3B7", "zeros"])
def test_the_sampler_samples_the_posterior(probabilities, name, seed):
    case, p = probabilities[name]
    K, B = case["K"], len(case["starts"]) - 1
    r = su.restate(case, 0, R_STAT, seed)
    assert r["sample_degenerate"] == 0
    code = (r["paths"].astype(np.int64) * (K ** np.arange(B))[None, :]).sum(1)
    count = np.bincount(code, minlength=K ** B).astype(np.float64)
    assert np.all(count[p == 0.0] == 0)                      # a path of probability 0 is never drawn
    small = R_STAT * p < 5.0
    cells_p = np.concatenate([p[~small], [p[small].sum()]])
    cells_n = np.concatenate([count[~small], [count[small].sum()]])
    dev = np.abs(cells_n - R_STAT * cells_p)
    bound = su.bernstein(R_STAT, cells_p)
    sigma = np.sqrt(np.maximum(R_STAT * cells_p * (1 - cells_p), 1e-300))
    worst = int(np.argmax(dev / bound))
    print("%s seed %d: %d cells, worst %.2f of the bound (%.2f sigma; the bound is at %.1f sigma there)"
          % (name, seed, len(cells_p), dev[worst] / bound[worst], dev[worst] / sigma[worst], bound[worst] / sigma[worst]))
    assert np.all(dev <= bound), (name, seed, worst, cells_n[worst], R_STAT * cells_p[worst])
    su.invariants(r, K, R_STAT, r["viterbi_score"], case["A"], case["pi"])

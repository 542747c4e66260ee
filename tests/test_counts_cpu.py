"""The count read-outs of the smoothing restated for one host thread (hammlet_amd/csrc/hml_counts_ref.h) as a stand-alone
program, tests/fixtures/counts_ref_main.cpp: built with g++ -Wall -Werror -ffp-contract=off, and a second time with the address
and undefined-behaviour sanitizers (nothing is loaded into Python for this), against the restatement in Python floats of
tests/counts_util.py.  Both sides derive every word from the same floats by the same IEEE operations in the same order, so (a)
compares words.

(b) compares the Python restatement - and, on the same cases, the program's words with it - with an enumeration of all K^B
paths, B <= 10 and K <= 3.  The bound is relative 1e-10 on every value above 1e-200: every operation of the recursions is on
non-negative numbers, so a value's relative error is bounded by the operation count of its longest chain times 2^-53 - the
smoothing's rows behind it included, here under 10^5 x 1.1e-16 - and never a measurement.  The reference is the enumeration.

(c) the histogram sums to 1 within (be - ba + 1) K 2^-50 where no boundary is degenerate, and the planted cases of
tests/infer_cases.py go through the sanitizer build with nothing on stderr and no not-a-number in any output."""
import math

import numpy as np
import pytest

from tests import counts_util as cu
from tests import infer_cases as ic
from tests import pairs_util as pz
from tests import posterior_util as pu


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    return cu.build_programs(tmp_path_factory.mktemp("counts_ref"))


# ---------------------------------------------------------------------------------------------- (a) word for word
def check_case(programs, case, H, what, names=("plain", "sanitized"), n_random=20):
    rng = np.random.default_rng(len(case["starts"]))
    start, end = pz.edge_regions(case["starts"], rng, n_random)
    t = cu.terms(case)
    want = cu.regions(case, t, start, end, H)
    for name in names:
        got = cu.run_program(programs[name], case, start, end, H)
        cu.same_terms(got, t, (what, name))
        assert np.array_equal(got["gamma"].ravel(), cu.words(np.array(t["gamma"]))), (what, name)
        assert got["count_degenerate"] == t["count_degenerate"], (what, name)
        assert (got["steps"], got["longest"]) == (want["steps"], want["longest"]), (what, name)
        cu.same_regions(got, cu.region_words(want), (what, name))
    return t, want, (start, end)


def check_sums_to_one(case, r, start, end, what):
    """(c): sum_h hist[h] = 1 within (be - ba + 1) K 2^-50"""
    starts = [int(v) for v in case["starts"]]
    for i, (a, e) in enumerate(zip(start, end)):
        n = pz.block_of(starts, int(e) - 1) - pz.block_of(starts, int(a))
        assert abs(math.fsum(r["hist"][i]) - 1.0) <= (n + 1) * case["K"] * 2.0 ** -50, (what, int(a), int(e))


@pytest.mark.parametrize("B", [1, 2, 3, 65, 120])
@pytest.mark.parametrize("K,H", [(2, 1), (2, 8), (3, 2), (3, 32), (5, 8)])
def test_every_word_equals_the_python_restatement(programs, K, H, B):
    rng = np.random.default_rng(1000 * K + 10 * H + B)
    case = pu.random_case(rng, K, B)
    t, r, (start, end) = check_case(programs, case, H, (K, H, B))
    assert t["count_degenerate"] == 0
    assert not any(t["v"][0]) and not any(t["rho"][0])
    check_sums_to_one(case, r, start, end, (K, H, B))
    if B == 1:
        g = np.array(t["gamma"][0])
        assert np.all(r["hist"][:, 0] == g.sum()) and not r["hist"][:, 1:].any()
        assert np.array_equal(r["whole_state"], np.broadcast_to(g, r["whole_state"].shape))
        assert np.allclose(r["avoid"], 1.0 - g, rtol=0, atol=1e-15)


def test_more_states_than_a_slice_word_for_word(programs):
    """17 states: two slices of the avoidance walk on the device; 64 with the largest max_breaks the rule allows there"""
    rng = np.random.default_rng(5)
    for K, H, B in [(17, 8, 20), (64, 15, 6)]:
        check_case(programs, pu.random_case(rng, K, B), H, (K, H, B), names=("plain",), n_random=3)


def test_two_dimensions_two_parameters_word_for_word(programs):
    rng = np.random.default_rng(7)
    for B in (65, 130):
        check_case(programs, pu.random_case(rng, 4, B, D=2, P=2), 8, ("D2", B))


def test_self_transitions_off_word_for_word(programs):
    rng = np.random.default_rng(8)
    for B in (64, 129):
        check_case(programs, pu.random_case(rng, 3, B, self_trans=False), 4, ("off", B))


def test_the_program_refuses_a_max_breaks_outside_the_rule(programs):
    import subprocess
    case = pu.random_case(np.random.default_rng(1), 64, 2)
    for H in (16, 0, 33):
        r = subprocess.run([programs["plain"]], input=cu.case_text(case, [0], [1], H), capture_output=True, text=True)
        assert r.returncode == 2 and "max_breaks must be 1 ... 32" in r.stdout, H
    assert cu.h_ok(64, 15) and not cu.h_ok(64, 16) and cu.h_ok(31, 32) and not cu.h_ok(32, 32) and cu.h_ok(16, 32)


# ---------------------------------------------------------------------------------------------- (b) all paths
REL = 1e-10
FLOOR = 1e-200


def block_regions(starts):
    """one region per pair of blocks ba <= be, its ends inside those blocks"""
    B = len(starts) - 1
    return [(int(starts[a]), int(starts[e + 1])) for a in range(B) for e in range(a, B)]


def close(got, ref, what):
    for x, y in zip(got, ref):
        if y > FLOOR or x > FLOOR:
            assert abs(x - y) <= REL * y, (what, x, y)


def check_against_all_paths(programs, case, H, what):
    want = cu.enumerate_counts(case)
    if want is None:
        return False
    K = case["K"]
    t = cu.terms(case)
    assert t["count_degenerate"] == 0, what
    rs = block_regions(case["starts"])
    for a, e in rs:
        got, ref = cu.region(case, t, a, e, H), want["counts"](a, e, H)
        assert (got["ba"], got["be"]) == (ref["ba"], ref["be"])
        for key in cu.REGION_KEYS:
            close(got[key], ref[key], (what, a, e, key))
        pair = want["region"](a, e)                 # the enumeration of tests/pairs_util.py: the same questions, asked there
        close(got["whole_state"], pair["whole_state"], (what, a, e, "pairs"))
        assert abs(got["hist"][0] - pair["whole"]) <= REL * pair["whole"] + FLOOR
        # the histogram's mean misses (n - H) of the paths with n > H breakpoints: at most (be - ba) hist[H]
        mean = math.fsum(h * got["hist"][h] for h in range(H + 1))
        assert abs(mean - pair["expected_breaks"]) <= (got["be"] - got["ba"]) * got["hist"][H] + 1e-12, (what, a, e)
        for x in range(K):                          # touching x and avoiding it partition the paths
            assert 0.0 <= got["avoid"][x] <= 1.0 + K * 2.0 ** -50
    start, end = np.array([r[0] for r in rs], np.uint32), np.array([r[1] for r in rs], np.uint32)
    got = cu.run_program(programs["plain"], case, start, end, H)          # the header's words are these
    cu.same_terms(got, t, what)
    cu.same_regions(got, cu.region_words(cu.regions(case, t, start, end, H)), what)
    return True


@pytest.mark.parametrize("seed", range(8))
def test_against_all_paths(programs, seed):
    rng = np.random.default_rng(4000 + seed)
    checked = 0
    while checked < 3:
        K, B = int(rng.integers(2, 4)), int(rng.integers(1, 9))
        H = int(rng.choice([1, 2, 3, 8]))
        case = pu.random_case(rng, K, B, max_len=3)
        if rng.random() < 0.3:
            A = case["A"].copy()
            i = int(rng.integers(K))
            A[i, (i + 1 + int(rng.integers(K - 1))) % K] = 0.0
            case["A"] = (A / A.sum(1, keepdims=True)).astype(np.float32)
        checked += check_against_all_paths(programs, case, H, (seed, K, B, H))


@pytest.mark.parametrize("K,B,H", [(3, 8, 8), (2, 10, 3), (3, 10, 2)])
def test_against_all_paths_at_the_largest_sizes(programs, K, B, H):
    """K = 3 with B = 8 under every pair (ba, be), and the bound's own corner B = 10; at B = 10 more breakpoints are possible
    than the histogram has bins, so the absorbing bin holds mass"""
    rng = np.random.default_rng(100 * K + B)
    case = pu.random_case(rng, K, B, max_len=2)
    assert check_against_all_paths(programs, case, H, (K, B, H))
    t = cu.terms(case)
    T = int(case["starts"][-1])
    whole = cu.region(case, t, 0, T, H)
    if B - 1 > H:
        assert whole["hist"][H] > 0.0


# ---------------------------------------------------------------------------------------------- (c) planted cases
@pytest.mark.parametrize("name", sorted(ic.CASES))
def test_planted_cases_hold_no_not_a_number(programs, name):
    """through the sanitizer build: nothing on stderr (run_program asserts it), no not-a-number in any output, every value a
    probability; where the case is in the table for degenerate boundaries of the pairwise read-outs, this one counts some too"""
    case = ic.case(name)
    K = case["K"]
    rng = np.random.default_rng(3)
    start, end = pz.edge_regions(case["starts"], rng, 10)
    for H in (1, 8):
        got = cu.run_program(programs["sanitized"], case, start, end, H)
        for key in ("v", "rho", "gamma") + cu.REGION_KEYS:
            a = got[key].view(np.float64)
            assert not np.isnan(a).any(), (name, H, key)
            assert (a >= 0.0).all() and np.isfinite(a).all(), (name, H, key)
        for key in cu.REGION_KEYS:
            assert (got[key].view(np.float64) <= 1.0 + 80 * K * 2.0 ** -50).all(), (name, H, key)
        if "pair_degenerate" in ic.EXPECT[name]:
            assert got["count_degenerate"] > 0, name
        if got["count_degenerate"] == 0:
            hist = got["hist"].view(np.float64)
            B = len(case["starts"]) - 1
            assert np.all(np.abs(hist.sum(axis=1) - 1.0) <= B * K * 2.0 ** -50), (name, H)

"""The pairwise read-outs of the smoothing restated for one host thread (hammlet_amd/csrc/hml_pairs_ref.h) as a stand-alone
program, tests/fixtures/pairs_ref_main.cpp: built with g++ -Wall -Werror -ffp-contract=off, and a second time with the address
and undefined-behaviour sanitizers (nothing is loaded into Python for this), against the restatement in Python floats and
integers of tests/pairs_util.py.  Both sides derive every word from the same floats by the same IEEE operations in the same
order, so (a) compares words.

(b) compares the Python restatement - and, on the same cases, the program's words with it - with an enumeration of all K^B
paths.  The bounds are the quantisation errors DESIGN.md derives plus the recursions' 1e-14, never a measurement:
whole_state within (be - ba) 2^-23 1.01 + 1e-12 relative, expected_breaks within (be - ba) 2^-33 + 1e-12, share within
2^-33 + 1e-12, p_b within 1e-12.  The reference is the enumeration."""
import math

import numpy as np
import pytest

from tests import em_util as eu
from tests import pairs_util as pz
from tests import posterior_util as pu


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    return pz.build_programs(tmp_path_factory.mktemp("pairs_ref"))


# ---------------------------------------------------------------------------------------------- (a) word for word
def check_case(programs, case, what, names=("plain", "sanitized"), n_random=40):
    rng = np.random.default_rng(len(case["starts"]))
    start, end = pz.edge_regions(case["starts"], rng, n_random)
    t = pz.terms(case)
    want = pz.region_words(pz.regions(case, t, start, end))
    for name in names:
        got = pz.run_program(programs[name], case, start, end)
        pz.same_terms(got, t, (what, name))
        assert np.array_equal(got["gamma"].ravel(), pz.words(np.array(t["gamma"]))), (what, name)
        assert got["pair_degenerate"] == t["pair_degenerate"] and got["total"] == t["N"][-1], (what, name)
        pz.same_regions(got, want, (what, name))
    return t, (start, end)


@pytest.mark.parametrize("B", [1, 2, 64, 65, 66, 200])
@pytest.mark.parametrize("K", [2, 3, 5])
def test_every_word_equals_the_python_restatement(programs, K, B):
    rng = np.random.default_rng(1000 * K + B)
    t, _ = check_case(programs, pu.random_case(rng, K, B), (K, B))
    assert t["pair_degenerate"] == 0
    assert t["p"][0] == 0.0 and t["pfx"][0] == 0 and not any(t["cost"][0])


@pytest.mark.parametrize("K", [2, 3, 5])
def test_a_long_trace_word_for_word(programs, K):
    rng = np.random.default_rng(77 + K)
    check_case(programs, pu.random_case(rng, K, 4098, max_len=2), (K, 4098), names=("plain",))


def test_two_dimensions_two_parameters_word_for_word(programs):
    rng = np.random.default_rng(7)
    for B in (65, 130):
        check_case(programs, pu.random_case(rng, 4, B, D=2, P=2), ("D2", B))


def test_self_transitions_off_word_for_word(programs):
    rng = np.random.default_rng(8)
    for B in (64, 129):
        check_case(programs, pu.random_case(rng, 3, B, self_trans=False), ("off", B))


# ---------------------------------------------------------------------------------------------- (b) all paths
def all_regions(starts):
    """every region whose ends lie on a block start or one position to either side of one"""
    T = int(starts[-1])
    cuts = sorted({min(max(int(s) + d, 0), T) for s in starts for d in (-1, 0, 1)})
    return [(a, e) for a in cuts for e in cuts if a < e]


@pytest.mark.parametrize("seed", range(8))
def test_against_all_paths(programs, seed):
    rng = np.random.default_rng(3000 + seed)
    checked = 0
    while checked < 4:
        K, B = int(rng.integers(2, 4)), int(rng.integers(1, 8))
        case = pu.random_case(rng, K, B, max_len=3)
        if rng.random() < 0.3:
            A = case["A"].copy()
            i = int(rng.integers(K))
            A[i, (i + 1 + int(rng.integers(K - 1))) % K] = 0.0
            case["A"] = (A / A.sum(1, keepdims=True)).astype(np.float32)
        want = pz.enumerate_pairs(case)
        if want is None:
            continue
        t = pz.terms(case)
        assert t["pair_degenerate"] == 0
        for b in range(B):
            assert abs(t["p"][b] - want["p"][b]) <= 1e-12, (K, B, b)
        rs = all_regions(case["starts"])
        for a, e in rs:
            got, ref = pz.region(case, t, a, e), want["region"](a, e)
            n = got["be"] - got["ba"]
            assert (got["ba"], got["be"]) == (ref["ba"], ref["be"])
            for j in range(K):
                assert abs(got["whole_state"][j] - ref["whole_state"][j]) <= (n * 2.0 ** -23 * 1.01 + 1e-12) * ref["whole_state"][j] + 1e-300, (K, B, a, e, j)
                assert abs(got["share"][j] - ref["share"][j]) <= 2.0 ** -33 + 1e-12, (K, B, a, e, j)
            assert abs(got["expected_breaks"] - ref["expected_breaks"]) <= n * 2.0 ** -33 + 1e-12, (K, B, a, e)
            assert abs(got["whole"] - ref["whole"]) <= (n * 2.0 ** -23 * 1.01 + 1e-12) * ref["whole"] + 1e-300, (K, B, a, e)
        start, end = np.array([r[0] for r in rs], np.uint32), np.array([r[1] for r in rs], np.uint32)
        got = pz.run_program(programs["plain"], case, start, end)          # the header's words are these
        pz.same_terms(got, t, (K, B))
        pz.same_regions(got, pz.region_words(pz.regions(case, t, start, end)), (K, B))
        checked += 1


# ---------------------------------------------------------------------------------------------- (c) identities
@pytest.fixture(scope="module")
def em_program(tmp_path_factory):
    return eu.build_programs(tmp_path_factory.mktemp("em_ref_for_pairs"), sanitized=False)["plain"]


def test_identities(programs, em_program):
    """on the words of the stand-alone program over hml_pairs_ref.h (which must be the Python restatement's), and for the last
    identity on the xi of hml_em_ref_estep as tests/fixtures/em_ref_main.cpp prints it"""
    rng = np.random.default_rng(31)
    for K, B, D, P in [(2, 70, 1, None), (3, 130, 1, None), (4, 40, 2, 2), (5, 65, 1, None)]:
        case = pu.random_case(rng, K, B, D=D, P=P)
        t = pz.terms(case)
        starts = [int(v) for v in case["starts"]]
        T = starts[-1]
        start, end = pz.edge_regions(starts, rng, 60)
        # 200 cuts a < m < e: the regions [a, m), [m, e) and [a, e) behind the others
        cuts = [sorted(rng.choice(T + 1, 3, replace=False).tolist()) for _ in range(200)]
        n0 = len(start)
        start = np.concatenate([start, [c[0] for c in cuts], [c[1] for c in cuts], [c[0] for c in cuts]]).astype(np.uint32)
        end = np.concatenate([end, [c[1] for c in cuts], [c[2] for c in cuts], [c[2] for c in cuts]]).astype(np.uint32)
        got = pz.run_program(programs["plain"], case, start, end)
        pz.same_terms(got, t, (K, B))
        pz.same_regions(got, pz.region_words(pz.regions(case, t, start, end)), (K, B))
        f64 = lambda key: got[key].view(np.float64)
        whole, whole_state, breaks, share, raw = f64("whole"), f64("whole_state"), f64("expected_breaks"), f64("share"), got["raw"].tolist()
        gamma, pfx, p = f64("gamma"), got["pfx"].tolist(), f64("p")
        for i in range(n0):
            a, e = int(start[i]), int(end[i])
            assert abs(math.fsum(share[i]) - 1.0) <= K * 2.0 ** -33, (K, B, a, e)
            ba, be = pz.block_of(starts, a), pz.block_of(starts, e - 1)
            if ba == be:      # inside one block
                assert raw[i][:1 + K] == [0] * (1 + K) and breaks[i] == 0.0
                s = 0.0
                for j in range(K):
                    assert whole_state[i, j] == gamma[ba, j]
                    s = s + gamma[ba, j]
                assert whole[i] == s
        # the raw break units add over two adjacent regions, plus pfx of the cut when the cut is a block start
        for k, (a, m, e) in enumerate(cuts):
            left, right, union = raw[n0 + k], raw[n0 + 200 + k], raw[n0 + 400 + k]
            at_start = m in starts
            assert left[0] + right[0] + (pfx[starts.index(m)] if at_start else 0) == union[0], (K, B, a, m, e)
            for j in range(K):      # and the masses add exactly
                assert left[1 + K + j] + right[1 + K + j] == union[1 + K + j], (K, B, a, m, e, j)
        # sum_b p_b = (B - 1) - trace(xi) of hml_em_ref_estep
        xi = eu.run_program(em_program, "estep", case)["xi"].view(np.float64).reshape(K, K)
        assert abs(math.fsum(p) - ((B - 1) - math.fsum(xi[j, j] for j in range(K)))) <= 1e-9
        assert abs(got["total"] * 2.0 ** -32 - math.fsum(p)) <= (B - 1) * 2.0 ** -33


# ---------------------------------------------------------------------------------------------- (d) defined edge behaviour
def test_a_zero_on_the_diagonal_caps_the_cost(programs):
    rng = np.random.default_rng(41)
    case = pu.random_case(rng, 3, 2, self_trans=False)        # (with self-transitions on, log A_jj = -inf lies inside E_b)
    case["A"] = np.array([[0.0, 0.5, 0.5], [0.25, 0.5, 0.25], [0.25, 0.25, 0.5]], np.float32)
    t = pz.terms(case)
    assert t["cost"][1][0] == pz.CAP and t["cost"][1][1] < pz.CAP and t["r"][1][0] == 0.0
    T = int(case["starts"][-1])
    r = pz.region(case, t, 0, T)
    assert r["whole_state"][0] == 0.0 and r["whole_state"][1] > 0.0
    got = pz.run_program(programs["sanitized"], case, [0], [T])
    pz.same_terms(got, t)
    pz.same_regions(got, pz.region_words(pz.regions(case, t, [0], [T])))


def test_an_unreachable_block(programs):
    """pi = (0, 1, 0), state 1 moves to state 0 alone, and the second block can only be state 2: no path reaches it.  The
    boundaries around it are counted as defined and no output holds a not-a-number"""
    starts = np.arange(7, dtype=np.uint32)
    x = np.array([0.0, 40.0, 40.0, 0.1, -0.1, 0.0], np.float32)
    A = np.array([[0.5, 0.25, 0.25], [1.0, 0.0, 0.0], [0.25, 0.25, 0.5]], np.float32)
    case = pu.make_case(3, starts, x, x * x, np.array([0.0, 1.0, 0.0, 1.0, 40.0, 1.0], np.float32), A, np.array([0.0, 1.0, 0.0], np.float32), self_trans=False)
    t = pz.terms(case)
    e_rows, m = pu.tables(case)
    s = pu.smooth(case, e_rows, m)
    assert s["degenerate"] == 1
    want_bad = 0
    for b in range(1, 6):       # the definition, once more, from the smoothing's rows
        v = [float(e_rows[b][j]) * s["beta"][b][j] for j in range(3)]
        X = 0.0
        for i in range(3):
            for j in range(3):
                X += (s["alpha"][b - 1][i] * float(A[i, j])) * v[j]
        want_bad += pz.bad(X)
    assert t["pair_degenerate"] >= 1 and t["pair_degenerate"] == want_bad
    rs = all_regions(starts)
    start, end = np.array([r[0] for r in rs], np.uint32), np.array([r[1] for r in rs], np.uint32)
    r = pz.regions(case, t, start, end)
    for key in ("whole", "whole_state", "expected_breaks", "share"):
        assert not np.isnan(r[key]).any(), key
    assert not np.isnan(np.array(t["p"])).any()
    for name, exe in programs.items():
        got = pz.run_program(exe, case, start, end)
        pz.same_terms(got, t, name)
        assert got["pair_degenerate"] == t["pair_degenerate"]
        pz.same_regions(got, pz.region_words(r), name)

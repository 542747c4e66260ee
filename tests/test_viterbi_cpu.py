"""The Viterbi restatement for one host thread (hammlet_amd/csrc/hml_viterbi_ref.h) as a stand-alone program,
tests/fixtures/viterbi_ref_main.cpp: built with g++ -Wall -Werror -ffp-contract=off, and a second time with the address and
undefined-behaviour sanitizers (nothing is loaded into Python for this), against the restatement in Python integers of
tests/viterbi_util.py.  Everything is compared for equality: the tables are integers by definition, and both sides derive them
from the same floats by the same IEEE operations in the same order.

Tie order, as include/hml.h states it: the smallest index wins in every back-pointer and in the end state, so of the paths
of maximal score the decode returns the one that is smallest when read from the LAST block backwards; the brute-force search
over all K^B paths finds exactly that one."""
import numpy as np
import pytest

from tests import viterbi_util as vu


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    return vu.build_programs(tmp_path_factory.mktemp("viterbi_ref"))


def sticky(K, stay=0.9):
    A = np.full((K, K), (1.0 - stay) / (K - 1), np.float32)
    np.fill_diagonal(A, stay)
    return A


def random_case(rng, K, B, D=1, P=None, self_trans=True, scale=1.0, max_len=5, twins=()):
    P = P or K
    lens = rng.integers(1, max_len + 1, B)
    starts = np.concatenate([[0], np.cumsum(lens)])
    level = rng.normal(0, 2, (D, B))
    sx = np.empty((D, B), np.float32)
    sq = np.empty((D, B), np.float32)
    for d in range(D):
        for b in range(B):
            x = (rng.normal(level[d, b], 1.0, lens[b]) * scale).astype(np.float32)
            sx[d, b] = x.sum(dtype=np.float32)
            sq[d, b] = (x * x).sum(dtype=np.float32)
    mean = np.sort(rng.normal(0, 2, P)).astype(np.float32)
    var = rng.uniform(0.3, 2.0, P).astype(np.float32)
    for a, b in twins:
        mean[b], var[b] = mean[a], var[a]
    mv = np.stack([mean, var], 1).ravel()
    A = rng.dirichlet(np.ones(K), K).astype(np.float32)
    pi = rng.dirichlet(np.ones(K)).astype(np.float32)
    return vu.make_case(K, starts, sx, sq, mv, A, pi, D=D, P=P, self_trans=self_trans)


def check(programs, case, what):
    """both builds against the Python restatement: tables, path, score; the score is the sum along the path"""
    emit, trans, init = vu.tables(case)
    path, score, psis, _ = vu.decode(emit, trans, init)
    for name, exe in programs.items():
        got = vu.run_case(exe, case)
        assert got["init"].tolist() == init, (what, name)
        assert got["trans"].tolist() == trans, (what, name)
        assert got["emit"].tolist() == emit, (what, name)
        assert got["path"].tolist() == path, (what, name)
        assert got["score"] == score, (what, name)
        assert got["score"] == vu.wrap64(vu.path_score(got["path"].tolist(), emit, trans, init)), (what, name)
    return emit, trans, init, path, score


@pytest.mark.parametrize("K,B,D,P,self_trans", [(2, 1, 1, None, True), (2, 2, 1, None, True), (3, 7, 1, None, True), (5, 40, 1, None, True),
                                                (5, 40, 1, None, False), (4, 33, 2, 2, True), (8, 20, 3, 2, True), (16, 12, 1, None, True),
                                                (20, 9, 1, None, True), (64, 5, 1, None, False)])
def test_tables_path_and_score(programs, K, B, D, P, self_trans):
    rng = np.random.default_rng(100 * K + B)
    check(programs, random_case(rng, K, B, D=D, P=P, self_trans=self_trans), (K, B, D))


def test_ties_go_to_the_lowest_index(programs):
    """states 1 and 2 are twins (same parameters, same rows and columns of A, same pi): every maximum they take part in is tied,
    in psi and at the end, and the path never holds the higher one; with all states equal the path is all zeros"""
    rng = np.random.default_rng(5)
    case = random_case(rng, 3, 60, twins=[(1, 2)])
    A = np.array([[0.8, 0.1, 0.1], [0.2, 0.4, 0.4], [0.2, 0.4, 0.4]], np.float32)
    case["A"], case["pi"] = A, np.array([0.5, 0.25, 0.25], np.float32)
    emit, trans, init, path, _ = check(programs, case, "twins")
    assert all(e[1] == e[2] for e in emit) and 1 in path and 2 not in path
    case = random_case(rng, 4, 30, twins=[(0, 1), (0, 2), (0, 3)])
    case["A"], case["pi"] = np.full((4, 4), 0.25, np.float32), np.full(4, 0.25, np.float32)
    assert check(programs, case, "all equal")[3] == [0] * 30


def test_zeros_in_A_and_pi(programs):
    """an exact 0 is log -inf, clamped to -2^38: a very bad transition that is still an ordinary number"""
    rng = np.random.default_rng(6)
    case = random_case(rng, 3, 50)
    case["A"] = np.array([[0.5, 0.5, 0.0], [0.0, 0.5, 0.5], [1.0, 0.0, 0.0]], np.float32)
    case["pi"] = np.array([0.0, 1.0, 0.0], np.float32)
    emit, trans, init, path, score = check(programs, case, "zeros")
    low = -(vu.LIM * vu.ONE)
    assert trans[0][2] == low and trans[2][1] == low and init[0] == low and init[2] == low and trans[2][0] == 0 and init[1] == 0
    assert path[0] == 1 and all((a, b) not in ((0, 2), (1, 0), (2, 1), (2, 2)) for a, b in zip(path, path[1:]))


def test_nonfinite_scores_are_clamped(programs):
    values = np.array([np.nan, np.inf, -np.inf, 3e38, -3e38, 0.0, -0.0, 1.0, -1.5, 2.0 ** 38, 2.0 ** 37, 2.0 ** -21, 3 * 2.0 ** -21, 5 * 2.0 ** -21,
                       -(2.0 ** -21), 1e-30], np.float32)
    want = [vu.fx(v) for v in values]
    top = vu.LIM * vu.ONE
    assert want[:7] == [-top, top, -top, top, -top, 0, 0] and want[9] == top and want[11:15] == [0, 2, 2, 0]   # (ties to even)
    for name, exe in programs.items():
        assert vu.run_fx(exe, values).tolist() == want, name
    # a negative entry of A: its logarithm is not a number
    rng = np.random.default_rng(7)
    case = random_case(rng, 2, 10)
    case["A"] = np.array([[0.5, -0.5], [0.5, 0.5]], np.float32)
    assert check(programs, case, "nan")[1][0][1] == -top


def test_data_scaled_by_2_to_the_40_clamps_every_term(programs):
    """every E is below -2^38: all emission words are equal, A and pi are symmetric, so every maximum is tied - state 0 throughout"""
    rng = np.random.default_rng(8)
    case = random_case(rng, 3, 25, scale=2.0 ** 40)
    case["A"], case["pi"] = sticky(3), np.full(3, 1 / 3, np.float32)
    emit, _, _, path, _ = check(programs, case, "scaled")
    assert all(v == -(vu.LIM * vu.ONE) for row in emit for v in row) and path == [0] * 25


@pytest.mark.parametrize("K,B,twins", [(2, 1, ()), (2, 6, ()), (3, 2, ()), (3, 5, ()), (3, 6, ()), (3, 6, [(0, 1)]), (3, 6, [(0, 1), (0, 2)]), (2, 6, [(0, 1)])])
def test_brute_force_over_all_paths(programs, K, B, twins):
    rng = np.random.default_rng(10 * K + B + len(twins))
    case = random_case(rng, K, B, twins=twins)
    if twins:
        case["A"], case["pi"] = sticky(K, 0.5) if len(twins) < K - 1 else np.full((K, K), 1 / K, np.float32), np.full(K, 1 / K, np.float32)
    emit, trans, init, path, score = check(programs, case, ("brute", K, B))
    best, arg = vu.brute_force(emit, trans, init)
    assert score == best and path == arg

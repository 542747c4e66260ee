"""EM from many starts (include/hml.h: hml_em_fit_many, hml_em_starts, hml_em_many_info, hml_set_em_batch_bytes) - what can be
checked without a GPU: the library's surface, the start generator and the winner's rule of hammlet_amd/csrc/hml_em_many_ref.h
(the functions the library calls, through tests/fixtures/em_many_ref_main.cpp, plain and under the sanitizers) against their
Python restatement word for word, and that the fixtures the GPU test reproduces are worth reproducing: on them several starts
end far apart, a generated start beats the given one, and members stop at different steps."""
import ctypes

import numpy as np
import pytest

from tests import em_many_util as mu
from tests import em_util as eu
from tests import posterior_util as pu

CALLS = ("hml_em_fit_many", "hml_em_starts", "hml_em_many_info", "hml_set_em_batch_bytes")
f32 = np.float32


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    return mu.build_programs(tmp_path_factory.mktemp("em_many"))


def test_library_exports_the_batch_calls():
    from hammlet_amd import build, capi
    build.build_library()
    lib = ctypes.CDLL(build.LIB_PATH)
    for name in CALLS:
        assert hasattr(lib, name), name
        assert name in capi.SIGNATURES
    for name in ("em_starts", "em_fit_many", "em_many_info", "set_em_batch_bytes"):
        assert hasattr(capi.Chain, name)


# ---------------------------------------------------------------------------------------------- starts
def _current(K, P, equal_means=False):
    rng = np.random.default_rng(100 * K + P)
    mean = np.full(P, 0.375, f32) if equal_means else rng.normal(0, 2, P).astype(f32)
    var = rng.uniform(0.05, 3.0, P).astype(f32)
    A = rng.dirichlet(np.ones(K), K).astype(f32)
    return np.stack([mean, var], 1).ravel(), A, rng.dirichlet(np.ones(K)).astype(f32)


STARTS = [(2, 2, False), (3, 3, False), (5, 5, False), (4, 2, False), (3, 3, True)]     # K, P (K = 4, P = 2: D = 2), equal current means


@pytest.mark.parametrize("K,P,equal", STARTS)
@pytest.mark.parametrize("R", (1, 2, 17))
def test_starts_equal_the_restatement(programs, K, P, equal, R):
    mv, A, pi = _current(K, P, equal)
    for seed in (5, 0xFEDCBA9876543210):
        for spread in (1.0, 0.3):
            want = mu.starts(K, P, R, seed, spread, mv, A, pi)
            for exe in programs.values():
                got = mu.program_starts(exe, K, P, R, seed, spread, mv, A, pi)
                for g, w in zip(got, want):
                    assert np.array_equal(g.ravel(), mu.words32(w).ravel()), (K, P, R, seed, spread)
            smv = want[0]
            assert np.array_equal(mu.words32(smv[0]), mu.words32(mv))                           # member 0 is the input
            assert np.all(np.diff(smv[1:, 0::2], axis=1) >= 0)                                  # the generated means ascend
            assert np.all(smv[:, 1::2] > 0) and np.all(np.isfinite(smv))
            assert all(np.array_equal(want[1][r], A) and np.array_equal(want[2][r], pi) for r in range(R))
    if R == 17:
        two = mu.starts(K, P, R, 5, 1.0, mv, A, pi)[0], mu.starts(K, P, R, 6, 1.0, mv, A, pi)[0]
        assert not np.array_equal(two[0][1:], two[1][1:])                                       # the seed matters
        assert len({m.tobytes() for m in two[0]}) == R                                          # and so does the member


def test_equal_current_means_fall_back_to_the_deviation():
    mv, A, pi = _current(3, 3, True)
    s = mu.starts(3, 3, 17, 9, 1.0, mv, A, pi)[0]
    h = float(np.sqrt(np.float64(mv[1::2].max())))
    assert np.ptp(s[1:, 0::2]) > 0.5 * h and np.all(np.abs(s[1:, 0::2].astype(np.float64) - 0.375) <= h * (1 + 1e-6))


@pytest.mark.parametrize("spread", (0.0, -1.0, float("inf"), float("nan")))
def test_a_bad_spread_is_refused(programs, spread):
    mv, A, pi = _current(3, 3)
    assert mu.starts(3, 3, 4, 1, spread, mv, A, pi) is None
    for exe in programs.values():
        assert mu.program_starts(exe, 3, 3, 4, 1, spread, mv, A, pi) is None


# ---------------------------------------------------------------------------------------------- the winner
WINNERS = {
    "greatest": ([1, 0, 1], [1.0, 3.0, 2.0], 1),
    "tie: the smallest index": ([1, 1, 0, 1], [2.0, 5.0, 5.0, 5.0], 1),
    "not-a-number": ([1, 1, 1], [float("nan"), -7.0, float("nan")], 1),
    "infinite": ([0, 0], [float("inf"), -1e300], 1),
    "a degenerate member with the greatest objective": ([1, eu.DEGENERATE, 0], [1.0, 9.0, 0.5], 0),
    "no candidate": ([eu.DEGENERATE, eu.DEGENERATE, 1], [1.0, 2.0, float("nan")], -1),
    "one member": ([0], [-3.5], 0),
    "negative zero ties with zero": ([1, 1], [-0.0, 0.0], 0),
}


@pytest.mark.parametrize("name", sorted(WINNERS))
def test_winner_rule(programs, name):
    reason, objective, want = WINNERS[name]
    assert mu.best(reason, objective) == want
    for exe in programs.values():
        assert mu.program_best(exe, reason, objective) == want


# ---------------------------------------------------------------------------------------------- multi-start does something
@pytest.fixture(scope="module")
def ragged(programs):
    out = {}
    for name in mu.RAGGED_CASES:
        case, mv, A, pi = mu.ragged_case(name)
        out[name] = (case, mv, A, pi) + mu.program_fits(programs["plain"], case, mv, A, pi, **mu.RAGGED)
    return out


def test_the_program_fits_as_the_python_restatement_does(ragged):
    """one member of each fixture: tests/em_util.py's fit from that start gives the program's words"""
    for name, r in (("k3", 4), ("k4", 1)):
        case, mv, A, pi, members, _ = ragged[name]
        fitted, trace, steps, reason, kept = eu.fit(dict(case, mean_var=mv[r], A=A[r], pi=pi[r]), mu.RAGGED["max_steps"], mu.RAGGED["rel_tol"])
        m = members[r]
        assert np.array_equal(m["trace"], eu.words(trace)) and (m["steps"], m["reason"], m["kept"]) == (steps, reason, kept)
        eu.same_parameters(m, fitted)


def test_starts_end_far_apart_at_three_states(ragged):
    members, win = ragged["k3"][4:]
    obj = [mu.objective_of(m) for m in members]
    assert all(m["reason"] != eu.DEGENERATE for m in members)
    assert max(obj) - min(obj) > 100.0
    assert obj[win] == max(obj) and win == obj.index(max(obj))


def test_a_generated_start_beats_the_given_one_at_four_states(ragged):
    members, win = ragged["k4"][4:]
    obj = [mu.objective_of(m) for m in members]
    assert win >= 1 and obj[win] > obj[0]


@pytest.mark.parametrize("name", sorted(mu.RAGGED_CASES))
def test_members_stop_at_different_steps(ragged, name):
    members = ragged[name][4]
    assert len({m["steps"] for m in members}) > 1
    assert all(len(m["trace"]) == m["steps"] + 1 for m in members)


def test_sanitized_program_fits(programs):
    """the sanitizer build over a short batch: the same words as the plain build"""
    case, mv, A, pi = mu.ragged_case("k3")
    case = pu.make_case(3, case["starts"][:41], case["sum"][0, :40], case["sum_sq"][0, :40], case["mean_var"], case["A"], case["pi"], self_trans=True)
    a = mu.program_fits(programs["plain"], case, mv[:3], A[:3], pi[:3], max_steps=3)
    b = mu.program_fits(programs["sanitized"], case, mv[:3], A[:3], pi[:3], max_steps=3)
    assert a[1] == b[1]
    for x, y in zip(a[0], b[0]):
        assert all(np.array_equal(x[k], y[k]) for k in x)

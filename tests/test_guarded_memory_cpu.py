"""What tests/test_gpu_guarded_memory.py runs under the guard mode, looked at on the CPU alone: the cases of the full-capacity
sweeps follow their rule, the fuzz slices are not hollow (tests/guarded_util.walk restates the draws of tests/fuzz_util._fuzz;
the GPU test holds every line that _fuzz logs against it), and the checker gives the hand-made recorder record what the test is
there for - every position a block, regions on the first and the last position, more history rows than two capacities.

Seeds of the slices (plain, tiny capacity, batched, compat, many states): 20270101, 20270201, 20270301, 20270401, 20270501.
A seed that misses a condition below is replaced; the thresholds stay."""
import numpy as np
import pytest

from tests import guarded_util as gu


def test_cases_follow_the_rule():
    """every length with at least two numbers of states on every path, every number of states at 1, 64, 65 and 1025"""
    assert gu.LENGTHS == [1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097]
    for lengths, states in ((gu.LENGTHS, gu.DEFAULT_K), (gu.LENGTHS, gu.MID_K), (gu.WEAK_LENGTHS, gu.WEAK_K), (gu.LENGTHS, gu.WIDE_K), (gu.LENGTHS, gu.COMPAT_K)):
        pairs = gu.spread(lengths, states)
        assert gu.covers(pairs, lengths, states), (lengths, states)
        assert len(pairs) == len(set(pairs))
    assert gu.DEFAULT_K == [2, 5, 7, 8, 16] and gu.WIDE_K == [17, 20, 64] and gu.COMPAT_K == [3, 20]
    assert not gu.covers([(T, 2) for T in gu.LENGTHS], gu.LENGTHS, gu.DEFAULT_K)


@pytest.mark.parametrize("name", ["plain", "compat", "wide"])
def test_fuzz_slices_are_not_hollow(name):
    n, seed, mode = gu.FUZZ_SLICES[name]
    records = gu.walk(n, seed, **mode)
    assert len(records) == n == {"plain": 40, "compat": 25, "wide": 30}[name]
    lines = [gu.line_of(c) for c in records]
    assert gu.wanting(lines) == []
    assert gu.walk(n, seed, **mode) == records                       # pure
    assert gu.walk(5, seed + 1, **mode) != records[:5]
    if name != "plain":
        assert sum(c["K"] > 16 for c in records) >= 3                # the paths that take the number of states at run time


def test_the_counts_of_the_slices():
    assert [gu.FUZZ_SLICES[k][0] for k in ("plain", "max_blocks_64", "many", "compat", "wide")] == [40, 25, 25, 25, 30]
    assert [n for n, _, _ in gu.FUZZ_HOSTILE] == [30, 10, 10, 10]
    assert [gu.READOUT_SLICES[k][0] for k in ("single_chain", "batched_chains", "many_states", "compat", "hostile")] == [15, 8, 8, 8, 10]
    seeds = [s for _, s, _ in list(gu.FUZZ_SLICES.values()) + gu.FUZZ_HOSTILE + list(gu.READOUT_SLICES.values())]
    assert len(set(seeds)) == len(seeds)


def test_wanting_sees_a_hollow_slice():
    full = ["  0 ok   T=17 K=4 D=2 dense=1 mult=1e+09 self=1 scheme=['S', 'P', ('F', 1, 1)]  B=17  0 s"] * 3
    assert gu.wanting(full) == []
    assert gu.wanting(full[:2]) == ["mult=1e+09 >= 3", "dense=1 >= 3"]
    assert gu.wanting([l.replace("D=2", "D=1").replace("'S', ", "") for l in full]) == ["D > 1 >= 2", "S in scheme >= 2"]


@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("T", gu.RECORDER_LENGTHS)
def test_the_checker_fills_the_recorders_record(oracle, T, D):
    from tests import readout_fuzz_util as rf
    c = gu.record_all(T, D=D)
    assert len(c["band_edges"][1]) == {2: 31, 3: 20}[D] and c["D"] == D and c["K"] == 2 ** D and c["every"] == 1 and all(c["on"][0].values())
    assert D * (len(c["band_edges"][1]) + 1) <= gu.BAND_COLUMNS < (D + 1) * (len(c["band_edges"][1]) + 1)
    exp = rf.expectations(c)
    reg = list(zip(exp["regions"][0].tolist(), exp["regions"][1].tolist()))
    assert (0, 1) in reg and (T - 1, T) in reg and (0, T) in reg
    assert len(exp["chains"][0]["rows"]) == 36 > 32                  # 16 rows, then 32, then 64: the buffer grows twice
    sweeps = [s for per_token in exp["chains"][0]["sweeps"] for s in per_token]
    assert len(sweeps) == 36 and all(len(s[0]) == T + 1 for s in sweeps), "every position a block"
    assert np.all(np.isfinite(exp["chains"][0]["theta"]))


@pytest.mark.parametrize("T,D", gu.VIEW_CASES)
def test_the_checker_accepts_the_records_of_the_dense_read_outs(oracle, T, D):
    from tests import readout_fuzz_util as rf
    c = gu.view_record(T, D)
    exp = rf.expectations(c)
    assert len(exp["chains"]) == (1 if D > 1 else 2)
    assert all(len(s[0]) == T + 1 for e in exp["chains"] for per_token in e["sweeps"] for s in per_token)

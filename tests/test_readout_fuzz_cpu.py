"""The sample of tests/test_gpu_readout_fuzz.py on the CPU CHECKER alone: the same generator (tests/readout_fuzz_util.generate, a
pure function), the same seeds and counts (readout_fuzz_util.SAMPLES), no GPU.  It shows that the sample covers what the GPU
test is there for and that the checker's sweeps give the recorders something to find.

Seeds (single chain, batched chains, many states, compat, hostile single + hostile batched):
    20261201, 20261202, 20261203, 20261204, 20261205 + 20261206
A seed that misses a line below is replaced; the thresholds stay."""
import numpy as np
import pytest

from tests import bands_util as bdu
from tests import breaks_util as bu
from tests import readout_fuzz_util as rf
from tests import regions_util as ru


@pytest.fixture(scope="module")
def records():
    out = []
    for name, parts in rf.SAMPLES.items():
        for n, seed, mode in parts:
            out += rf.generate(n, seed, **mode)
    return out


@pytest.fixture(scope="module")
def checked(records):
    """(record, expectations or the refusal's message) of every record: the checker runs once per module"""
    out = []
    for c in records:
        try:
            out.append((c, rf.expectations(c)))
        except rf.Refused as err:
            out.append((c, str(err)))
    return out


def test_the_generator_is_pure():
    a = rf.generate(6, 20261201)
    b = rf.generate(6, 20261201)
    assert a == b and rf.generate(6, 20261201, only=4) == [a[4]]
    assert rf.generate(3, 20261202, many=True) != a[:3]


def _ever_on(c, r):
    return any(any(flags[r]) for flags in rf.on_by_token(c))


def test_coverage_of_the_sample(records):
    assert len(records) == 40 + 15 + 15 + 15 + 20 + 8
    for r in rf.RECORDERS:
        assert sum(_ever_on(c, r) for c in records) >= 10, r
    assert sum(max(sum(on.values()) for on in c["on"]) >= 4 for c in records) >= 10
    assert sum(bool(c["flips"]) for c in records) >= 5
    assert sum(bool(c["midrun"]) for c in records) >= 10
    # graph replay: single chains outside compat mode only (hml_iterate_many and compat contexts run eagerly whatever the switch
    # says); a replayed graph holds sweeps that are not recorded, so these are recorded sweeps run eagerly BETWEEN replayed ones
    assert sum(c["env"].get("HML_USE_GRAPH") == 1 and not c["many"] and not c["compat"] for c in records) >= 5
    assert sum(any(k in c["midrun"] for k, tok in enumerate(c["scheme"]) if not isinstance(tok, tuple)) for c in records) >= 5    # behind S, D or P
    assert sum(any(not f[2] for f in c["flips"].values()) for c in records) >= 3       # a switch behind sweeps still enqueued
    assert sum(c["max_blocks"] == 64 or c["env"].get("HML_MAX_BLOCKS") == 64 for c in records) >= 8
    assert sum(c["dense"] for c in records) >= 8
    assert sum(any(isinstance(tok, tuple) and tok[2] > 0 and tok[1] % tok[2] != 0 for tok in c["scheme"]) for c in records) >= 5
    assert {c["T"] for c in records if c["T"] is not None} == set(rf.T_LIST)
    assert sum(c["many"] and len({tuple(sorted(on.items())) for on in c["on"]}) > 1 for c in records) >= 3
    # every kind of mid-run read-out and every recorder's switch occurs
    assert {m[1] for c in records for m in c["midrun"].values()} == set(rf.READOUTS)
    assert {f[1] for c in records for f in c["flips"].values()} == set(rf.RECORDERS)


def _first_chain_with(exp, r):
    for chain in range(len(exp["chains"])):
        sweeps = rf.sweeps_of(exp, chain, r)
        if sweeps:
            return chain, sweeps
    return None, []


def test_the_checker_gives_the_recorders_something_to_find(checked):
    recording, two_sweeps, partial_break = 0, 0, 0
    with_bands, two_bands, with_regions, whole_and_cut = 0, 0, 0, 0
    for c, exp in checked:
        if isinstance(exp, str):
            continue
        T = exp["T"]
        every = [s for per_token in exp["chains"][0]["sweeps"] for s in per_token]
        if not every:
            continue
        recording += 1
        N = len(every)
        two_sweeps += N >= 2
        C, _ = bu.counts(every, T)
        partial_break += bool(np.any((C > 0) & (C < N)))
        chain, sweeps = _first_chain_with(exp, "bands")
        if sweeps:
            with_bands += 1
            nb = len(exp["case"]["edges"]) + 1
            counts, _, _ = bdu.accumulate(sweeps, T, exp["case"]["edges"], D=c["D"], P=(c["P"] if c["D"] > 1 else c["K"]))
            two_bands += bool(any(np.any((counts[d * nb:(d + 1) * nb] > 0).sum(axis=0) >= 2) for d in range(c["D"])))
        chain, sweeps = _first_chain_with(exp, "regions")
        if sweeps:
            with_regions += 1
            want = ru.accumulate(sweeps, exp["regions"][0], exp["regions"][1], exp["region_edges"], D=c["D"], P=(c["P"] if c["D"] > 1 else None))
            whole_and_cut += bool(np.any(want["whole"] == want["N"]) and np.any(want["whole"] < want["N"]))
    print("recording %d: N >= 2 in %d, a breakpoint count inside (0, N) in %d; bands %d: two bands at a position in %d; regions %d: whole and cut in %d"
          % (recording, two_sweeps, partial_break, with_bands, two_bands, with_regions, whole_and_cut))
    assert recording >= 60
    assert two_sweeps >= 0.6 * recording
    assert partial_break >= 0.5 * recording
    assert with_bands >= 20 and two_bands >= 0.5 * with_bands
    assert with_regions >= 20 and whole_and_cut >= 0.5 * with_regions


def test_hardly_any_configuration_is_left_out(checked):
    """`both raise` - the reference's refusal at the auto prior - leaves a configuration unchecked: none on Gaussian and
    read-depth data (T >= 33 there), at most 15 % on hostile data"""
    refused = [(c, exp) for c, exp in checked if isinstance(exp, str)]
    for c, message in refused:
        print("both raise: %s  %s" % (message, rf.describe(c)))
    assert not [c for c, _ in refused if not c["hostile"]]
    hostile = [c for c, _ in checked if c["hostile"]]
    assert len([c for c, _ in refused if c["hostile"]]) <= 0.15 * len(hostile)

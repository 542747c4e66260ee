"""The sample of tests/test_gpu_infer_fuzz.py without a GPU: the same generator (tests/infer_fuzz_util.generate, a pure function),
the same seed and count (infer_fuzz_util.SAMPLE).  It shows that the sample covers what the GPU test is there for, and - where a
configuration's case does not depend on a chain's sweeps - that the smoothing restatement (the stand-alone program over
hammlet_amd/csrc/hml_posterior_ref.h) on the ideal statistics finds degenerate blocks.  A seed that misses a line below is
replaced; the thresholds stay."""
import pytest

from tests import infer_fuzz_util as fu
from tests import posterior_util as pu


@pytest.fixture(scope="module")
def records():
    return fu.generate(*fu.SAMPLE)


def test_the_generator_is_pure():
    a, b = fu.generate(6, 20261301), fu.generate(6, 20261301)
    assert a == b and fu.generate(6, 20261301, only=4) == [a[4]]
    assert fu.generate(3, 20261302) != a[:3]


def test_coverage_of_the_sample(records):
    assert {c["K"] for c in records if not c["dims"]} == set(fu.KS)
    assert any(c["dims"] == (2, 2) for c in records) and any(not c["dims"] for c in records)
    assert {c["every_position"] for c in records} == {False, True}
    assert {c["kind"] for c in records} == set(fu.KINDS)
    assert {c["self_trans"] for c in records} == {False, True} and {c["zeros"] for c in records} == {False, True}
    assert {c["sweeps"] for c in records} == set(range(6)) and {c["params"] for c in records} == set(fu.PARAMS)
    assert {c["T"] for c in records} >= {1, 2, 65, 1000, 4097}
    for p in ("viterbi", "posterior", "sample"):
        assert {c["geometry"][p][0] for c in records} == {1, 4, 64, 1024} and {c["geometry"][p][2] for c in records} == {0, 1, 8}, p


def test_a_tenth_of_the_sample_has_degenerate_blocks(records, tmp_path):
    program = pu.build_programs(tmp_path, sanitized=False)["plain"]
    degenerate = 0
    for c in records:
        case = fu.ideal_case(c)
        if case is not None:
            degenerate += pu.run_case(program, case, want_rows=False)["degenerate"] > 0
    assert 10 * degenerate >= len(records), (degenerate, len(records))

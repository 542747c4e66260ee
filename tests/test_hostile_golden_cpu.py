"""The CPU checker (oracle/) in reference mode against files the unmodified reference binary wrote for inputs that are not a
unit-scale Gaussian trace (tests/hostile_inputs.py; tests/golden/hostile/, made by tests/golden/make_hostile_golden.py: a manifest of checksums and an archive of the files): scaled
by 2^+-10, 2^+-40, 10^+-3, shifted by 10 / 100 / 1000, read depths of 1 to 5000 with 3 to 20 states, integer data full of ties,
spikes, 2 to 65 positions, two read-depth runs of 10^6 positions - byte for byte; and the reference's message and exit status
for the inputs it refuses.  The GPU tests of tests/test_gpu_hostile.py compare the product with the checker on the same
inputs: this file is what ties the checker to the reference there."""
import pytest

from tests import hostile_inputs as hi
from tests.test_oracle_golden import run_cli

MANIFEST = hi.manifest()
RUN = sorted(c for c in MANIFEST if MANIFEST[c]["status"] == 0)


def test_every_input_has_a_golden_run():
    assert sorted(MANIFEST) == sorted(list(hi.INPUTS) + list(hi.MILLION))
    assert sorted(c for c in MANIFEST if MANIFEST[c]["status"] != 0) == hi.REFUSED
    for fam in ("scale", "offset", "depth", "ties", "spikes", "tiny"):
        assert hi.family(fam)


@pytest.mark.parametrize("case", RUN)
def test_reference_mode_reproduces_reference_files_on_hostile_inputs(case):
    m = MANIFEST[case]
    out, stdout = run_cli(case, manifest=MANIFEST, x=hi.golden_input(m, case))
    for o in m["outputs"]:
        hi.assert_golden(m, case, o, out[o].encode())
    assert stdout == m["stdout"]


@pytest.mark.parametrize("case", ["scale_2m40", "ties_plateaus_noise"])
def test_restated_distributions_reproduce_reference_files_on_hostile_inputs(case):
    """--rng 3: the mt19937 stream through the restated categorical / gamma / normal of hml_dist.h (the code that runs on the
    GPU): at x 2^-40 rows of the backward draw underflow to all zeros - the categorical draw then returns index 0 like
    libstdc++'s - and the integer plateaus give exactly equal weights."""
    m = MANIFEST[case]
    out, _ = run_cli(case, ["--rng", "3"], manifest=MANIFEST, x=hi.golden_input(m, case))
    for o in m["outputs"]:
        hi.assert_golden(m, case, o, out[o].encode())


@pytest.mark.parametrize("case", hi.REFUSED)
def test_refused_inputs_give_the_references_message_and_status(case):
    m = dict(MANIFEST[case], outputs=hi.SMALL_OUTPUTS)
    _, stdout, r = run_cli(case, manifest={case: m}, x=hi.golden_input(m, case), check=False)
    assert r.returncode == m["status"] != 0
    assert r.stderr == m["stderr"]
    assert stdout == m["stdout"]

"""A bounded, fixed-seed sample of the randomised differential run of the exact-inference passes (tests/infer_fuzz_util.py): a
configuration draws its data (ol.trace or a member of hostile_inputs.fuzz_draw), 1 to 4097 positions, 2 to 64 states or two data
dimensions over two parameters, self-transitions on or off, every position a block or the chain's own threshold, 0 to 5 sweeps,
the chain's parameters or planted ones (unit-scale; every variance but the first at the smallest denormal), optionally zeros in A and pi, and a
geometry per pass; then the Viterbi decode, the smoothing, the expected counts, two fits, EM from three starts, the pairwise
read-outs and eight sampled paths go against the stand-alone restatements, word for word.

tests/test_infer_fuzz_cpu.py shows without a GPU what the sample covers.  A failure names the configuration:
    python tools/fuzz_infer.py --seed S --only I

Wall time on one MI355X, measured once: 7.3 s for the 56 configurations (the four tests 4.4, 1.2, 1.1 and 0.6 s; the programs'
text takes most of it), tests/test_gpu_readout_fuzz.py next to it 11.8 s."""
import pytest

from tests.infer_fuzz_util import SAMPLE, build_programs, fuzz_infer

pytestmark = pytest.mark.gpu
PARTS = 4


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    return build_programs(tmp_path_factory.mktemp("infer_fuzz"))


@pytest.mark.parametrize("part", range(PARTS))
def test_infer_fuzz(hml, programs, part):
    n, seed = SAMPLE
    for i in range(part, n, PARTS):
        assert fuzz_infer(hml, programs, n, seed, log=print, only=i) == 1

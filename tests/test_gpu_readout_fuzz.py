"""A bounded, fixed-seed sample of the randomised differential run of the RECORDINGS (tests/readout_fuzz_util.py): several
recorders on at once - state marginals, emission levels, breakpoints and their consensus, level bands, regions, history - in a
chain that goes through a random scheme of M / F / S / D / P tokens on every switchable sweep path (both forward geometries,
the trellis switches, graph replay, block capacities of 64, compat mode, the path for many states), with thinnings that do not
divide a token, recorders switched on and off between tokens and read-outs taken in mid-run; at the end of a configuration the
chain itself (blocks, states, parameter and transition bits, marginals text), then every recorder through the helper of its
own test file against the CPU checker's recorded sweeps, one dense form, with probability 0.3 the three payloads into a fresh
context and a Viterbi decode against the stand-alone restatement.  Batches: 2-10 chains through hml_iterate_many, each with a
recorder set of its own, then the agreement of the chains that recorded levels and the merges of chain 1 into chain 0.

tests/test_readout_fuzz_cpu.py shows on the checker alone what the sample covers.  A failure names the configuration:
    python tools/fuzz_readouts.py --seed S --only I [many|wide|compat] [hostile]

Wall time of each test on one MI355X (the call phase; torch is imported when this module is collected, as a run of the whole
suite has done long before it gets here), measured once:
    single_chain 3.1 s, batched_chains 5.7 s, many_states 1.1 s, compat 1.2 s, hostile 0.7 s"""
import pytest
import torch  # noqa: F401  (the dense forms and the payloads go through torch buffers: imported at collection, not inside the first test)

from tests.readout_fuzz_util import SAMPLES, fuzz_readouts

pytestmark = pytest.mark.gpu


def _run(hml, name):
    for n, seed, mode in SAMPLES[name]:
        assert fuzz_readouts(hml, n, seed, **mode) == n


def test_readout_fuzz_single_chain(hml):
    _run(hml, "single_chain")


def test_readout_fuzz_batched_chains(hml):
    _run(hml, "batched_chains")


def test_readout_fuzz_many_states(hml):
    _run(hml, "many_states")


def test_readout_fuzz_compat(hml):
    """the reference-compatible mode against the checker's REFERENCE mode"""
    _run(hml, "compat")


def test_readout_fuzz_hostile(hml):
    """inputs of tests/hostile_inputs.py, 2 to 65537 positions: single chains, then batches"""
    _run(hml, "hostile")

"""`hammlet -O V` (viterbi; extension): PREFIXviterbiSUFFIX holds, in the maxsegmentation file's format, the runs that the
restatement for one host thread (tests/fixtures/viterbi_ref_main.cpp) decodes from the blocks, block statistics and final
parameters of the chain of the same seed and chain number; with -chains 2 there is one file per chain."""
import os

import pytest

from tests.cli_util import run_cli
from tests import oracle_lib as ol
from tests import viterbi_util as vu

pytestmark = pytest.mark.gpu
T, K, SEED = 30000, 3, 4
SCHEME = [("M", 4, 0), ("F", 36, 0)]
FLAGS = "-s %d -R %d -i M 4 0 F 36 0" % (K, SEED)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return vu.build_programs(tmp_path_factory.mktemp("viterbi_ref"), sanitized=False)["plain"]


def want_text(hml, program, x, chain_id):
    g = hml.Chain(device=0, seed=SEED, chain_id=chain_id)
    g.load(x)
    g.set_model(K, g.autoprior(0.2, 0.9))
    g.sample_prior()
    for m, n, t in SCHEME:
        g.iterate(m, n, t)
    g.sync()
    case = vu.chain_case(g)
    want = vu.run_case(program, case, want_emit=False)
    text = vu.tool_text(*vu.runs_of(want["path"], case["starts"]))
    assert sum(int(l.split("\t")[0]) for l in text.splitlines()) == T
    return text


def test_viterbi_file(hml, program, tmp_path):
    x = ol.trace(T, K, 7)
    r = run_cli(str(tmp_path), x, FLAGS, ["V"])
    assert r.returncode == 0, r.stderr
    assert open(str(tmp_path / "g-viterbi.csv")).read() == want_text(hml, program, x, 0)
    assert not os.path.exists(str(tmp_path / "g-marginals.csv"))
    # the long name, next to another output; an existing file is refused without -w
    r = run_cli(str(tmp_path), x, FLAGS, ["viterbi", "X"], overwrite=False)
    assert r.returncode != 0 and "g-viterbi.csv already exists" in r.stderr + r.stdout


def test_viterbi_files_of_two_chains(hml, program, tmp_path):
    x = ol.trace(T, K, 8)
    r = run_cli(str(tmp_path), x, FLAGS + " -chains 2", ["V"])
    assert r.returncode == 0, r.stderr
    assert open(str(tmp_path / "g-viterbi.csv")).read() == want_text(hml, program, x, 0)
    assert open(str(tmp_path / "g-chain1.viterbi.csv")).read() == want_text(hml, program, x, 1)

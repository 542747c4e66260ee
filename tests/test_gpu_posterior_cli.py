"""`hammlet -O PD` (posterior; extension): PREFIXposteriorSUFFIX holds log p(y | theta) and the degenerate count, then per run
length, state and confidence - what Chain.posterior() and Chain.posterior_rle() give for the chain of the same seed and chain
number after the same scheme; with -chains 2 there is one file per chain."""
import os

import pytest

from tests.cli_util import run_cli
from tests import oracle_lib as ol
from tests import posterior_util as pu

pytestmark = pytest.mark.gpu
T, K, SEED = 30000, 3, 4
SCHEME = [("M", 4, 0), ("F", 36, 0)]
FLAGS = "-s %d -R %d -i M 4 0 F 36 0" % (K, SEED)


def want_text(hml, x, chain_id):
    g = hml.Chain(device=0, seed=SEED, chain_id=chain_id)
    g.load(x)
    g.set_model(K, g.autoprior(0.2, 0.9))
    g.sample_prior()
    for m, n, t in SCHEME:
        g.iterate(m, n, t)
    g.sync()
    _, loglik, degenerate = g.posterior()
    run_len, run_state, run_conf = g.posterior_rle()
    assert int(run_len.sum()) == T and degenerate == 0
    return pu.tool_text(loglik, degenerate, run_len, run_state, run_conf)


def test_posterior_file(hml, tmp_path):
    x = ol.trace(T, K, 7)
    r = run_cli(str(tmp_path), x, FLAGS, ["PD"])
    assert r.returncode == 0, r.stderr
    text = open(str(tmp_path / "g-posterior.csv")).read()
    assert text == want_text(hml, x, 0)
    lines = text.splitlines()
    assert len(lines[0].split("\t")) == 2 and all(len(l.split("\t")) == 3 and 0.0 <= float(l.split("\t")[2]) <= 1.0 for l in lines[1:])
    assert not os.path.exists(str(tmp_path / "g-marginals.csv"))
    # the long name, next to another output; an existing file is refused without -w
    r = run_cli(str(tmp_path), x, FLAGS, ["posterior", "X"], overwrite=False)
    assert r.returncode != 0 and "g-posterior.csv already exists" in r.stderr + r.stdout
    # a scheme of mixture sweeps alone has no transitions to sum over
    r = run_cli(str(tmp_path), x, "-s %d -R %d -i M 4 0" % (K, SEED), ["PD"])
    assert r.returncode != 0 and "mixture sweeps only" in r.stderr + r.stdout


def test_posterior_files_of_two_chains(hml, tmp_path):
    x = ol.trace(T, K, 8)
    r = run_cli(str(tmp_path), x, FLAGS + " -chains 2", ["PD"])
    assert r.returncode == 0, r.stderr
    assert open(str(tmp_path / "g-posterior.csv")).read() == want_text(hml, x, 0)
    assert open(str(tmp_path / "g-chain1.posterior.csv")).read() == want_text(hml, x, 1)

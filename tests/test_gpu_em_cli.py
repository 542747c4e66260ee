"""`hammlet -em STEPS [TOL] [-em-prior] -O EM` (extension): the fit runs once the scheme has run and before the end-of-run
outputs, so PREFIXviterbiSUFFIX and PREFIXposteriorSUFFIX are under the fitted parameters; PREFIXemSUFFIX holds the trace that
Chain.em_fit gives for the chain of the same seed after the same scheme.  The shape is the baseline's config 1."""
import os

import pytest

from tests.cli_util import run_cli
from tests import oracle_lib as ol

pytestmark = pytest.mark.gpu
T, K, SEED = 100000, 3, 1
FLAGS = "-s %d -R %d -i F 100 1" % (K, SEED)


def fitted_chain(hml, x, steps, use_prior):
    g = hml.Chain(device=0, seed=SEED)
    g.load(x)
    g.set_model(K, g.autoprior(0.2, 0.9))
    g.sample_prior()
    g.iterate("F", 100, 1)
    g.sync()
    return g, g.em_fit(steps, use_prior=use_prior)


@pytest.mark.parametrize("use_prior", [False, True])
def test_em_file_and_the_outputs_under_the_fit(hml, tmp_path, use_prior):
    x = ol.trace(T, K, 7)
    r = run_cli(str(tmp_path), x, FLAGS + " -em 10" + (" -em-prior" if use_prior else ""), ["EM", "V", "PD"])
    assert r.returncode == 0, r.stderr
    for name in ("em", "viterbi", "posterior"):
        assert os.path.exists(str(tmp_path / ("g-%s.csv" % name))), name
    lines = open(str(tmp_path / "g-em.csv")).read().splitlines()
    g, (trace, steps, reason, kept) = fitted_chain(hml, x, 10, use_prior)
    want = ["%d\t%.17g" % (k, v) for k, v in enumerate(trace)]
    assert lines[:len(want)] == want and steps >= 1 and trace[-1] > trace[0]
    rest = lines[len(want):]
    assert rest[0] == "reason\t" + {hml.EM_MAX_STEPS: "max_steps", hml.EM_CONVERGED: "converged", hml.EM_DEGENERATE: "degenerate"}[reason]
    assert rest[1] == "kept\t%d" % kept
    mv, (A, pi) = g.theta(), g.transitions()
    fmt = lambda name, v: "\t".join([name] + ["%.9g" % float(t) for t in v])
    assert rest[2] == fmt("means", mv[0::2]) and rest[3] == fmt("variances", mv[1::2])
    assert rest[4:4 + K] == [fmt("A", row) for row in A] and rest[4 + K] == fmt("pi", pi) and len(rest) == 5 + K
    # the posterior file is under the fitted parameters: its log-likelihood is the chain's after the same fit
    first = open(str(tmp_path / "g-posterior.csv")).readline().split("\t")
    assert first[0] == "%.17g" % g.posterior()[1]
    if not use_prior:
        assert first[0] == "%.17g" % trace[-1]               # ... and the last trace entry


def test_refusals(tmp_path):
    x = ol.trace(2000, K, 7)
    r = run_cli(str(tmp_path), x, "-s %d -R %d -i M 4 0 -em 5" % (K, SEED), ["EM"])
    assert r.returncode == 1 and "[ERROR] The fit (-em) needs a model with transitions: the scheme has mixture sweeps only!" in r.stderr
    r = run_cli(str(tmp_path), x, FLAGS, ["EM"])
    assert r.returncode == 1 and "[ERROR] The output em (EM) needs a fit" in r.stderr
    assert not os.path.exists(str(tmp_path / "g-em.csv"))

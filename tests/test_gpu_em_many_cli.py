"""`hammlet -em STEPS [TOL] -em-starts R [SEED [SPREAD]] -O EM EMS` (extension): the fit of -em becomes a batch from R starts whose
winner is installed.  PREFIXemstartsSUFFIX holds one line per member and PREFIXemSUFFIX the winner's trace, both what
Chain.em_fit_many gives for the chain of the same seed after the same scheme; one start is the single fit's files byte for byte."""
import os

import pytest

from tests import oracle_lib as ol
from tests.cli_util import run_cli
from tests.test_gpu_em_cli import FLAGS, K, SEED

pytestmark = pytest.mark.gpu
T, R, STARTS_SEED, STEPS = 30000, 5, 7, 6
REASON = {0: "max_steps", 1: "converged", 2: "degenerate"}


def scheme_chain(hml, x):
    g = hml.Chain(device=0, seed=SEED)
    g.load(x)
    g.set_model(K, g.autoprior(0.2, 0.9))
    g.sample_prior()
    g.iterate("F", 100, 1)
    g.sync()
    return g


def test_the_batch_s_files(hml, tmp_path):
    x = ol.trace(T, K, 7)
    r = run_cli(str(tmp_path), x, FLAGS + " -em %d -em-starts %d %d 1.5" % (STEPS, R, STARTS_SEED), ["EM", "EMS", "PD"])
    assert r.returncode == 0 and r.stderr == "", r.stderr
    g = scheme_chain(hml, x)
    got = g.em_fit_many(n_starts=R, seed=STARTS_SEED, spread=1.5, max_steps=STEPS)
    win = got["best"]
    assert win >= 0
    fmt = lambda v: ["%.9g" % float(t) for t in v]
    want = []
    for m in range(R):
        fields = ["%d" % m, "%.17g" % got["objective"][m], "%d" % got["steps"][m], REASON[int(got["reason"][m])], "%d" % got["kept"][m]]
        want.append("\t".join(fields + fmt(got["mean_var"][m][0::2]) + fmt(got["mean_var"][m][1::2]) + (["*"] if m == win else [])))
    assert open(str(tmp_path / "g-emstarts.csv")).read().splitlines() == want
    # the em file is the winner's, in the single fit's format, and the parameters in it are the installed ones
    lines = open(str(tmp_path / "g-em.csv")).read().splitlines()
    n = int(got["steps"][win]) + 1
    assert lines[:n] == ["%d\t%.17g" % (k, v) for k, v in enumerate(got["trace"][win][:n])]
    assert lines[n] == "reason\t" + REASON[int(got["reason"][win])] and lines[n + 1] == "kept\t%d" % got["kept"][win]
    assert lines[n + 2] == "\t".join(["means"] + fmt(got["mean_var"][win][0::2])) and lines[n + 3] == "\t".join(["variances"] + fmt(got["mean_var"][win][1::2]))
    assert lines[n + 4:n + 4 + K] == ["\t".join(["A"] + fmt(row)) for row in got["A"][win]] and lines[n + 4 + K] == "\t".join(["pi"] + fmt(got["pi"][win]))
    # the end-of-run outputs are under the winner's parameters
    assert open(str(tmp_path / "g-posterior.csv")).readline().split("\t")[0] == "%.17g" % g.posterior()[1]


def test_one_start_is_the_single_fit(tmp_path):
    """without -em-starts nothing changes; with one start - the chain's own parameters - the files are the single fit's, byte for byte"""
    x = ol.trace(T, K, 7)
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir(); b.mkdir()
    ra = run_cli(str(a), x, FLAGS + " -em %d" % STEPS, ["EM", "V", "PD"])
    rb = run_cli(str(b), x, FLAGS + " -em %d -em-starts 1" % STEPS, ["EM", "V", "PD"])
    assert ra.returncode == 0 and rb.returncode == 0, (ra.stderr, rb.stderr)
    assert sorted(os.listdir(str(a))) == sorted(os.listdir(str(b)))
    for name in ("g-em.csv", "g-viterbi.csv", "g-posterior.csv"):
        assert open(str(a / name), "rb").read() == open(str(b / name), "rb").read(), name


def test_refusals(tmp_path):
    x = ol.trace(2000, K, 7)
    r = run_cli(str(tmp_path), x, FLAGS + " -em-starts 4", ["M"])
    assert r.returncode == 1 and "[ERROR] The flag -em-starts needs a fit" in r.stderr
    r = run_cli(str(tmp_path), x, FLAGS + " -em 3", ["EMS"])
    assert r.returncode == 1 and "[ERROR] The output emstarts (EMS) needs a batch" in r.stderr
    for bad in ("0", "4097", "2.5", "3 1.5", "3 1 0", "3 1 2 4"):
        r = run_cli(str(tmp_path), x, FLAGS + " -em 3 -em-starts " + bad, ["EMS"])
        assert r.returncode == 1 and "-em-starts" in r.stderr, bad
    assert not os.path.exists(str(tmp_path / "g-emstarts.csv"))

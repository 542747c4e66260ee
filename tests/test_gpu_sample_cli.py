"""`hammlet -psample R [SEED] -O PS -O PSS` (extension): the draws are made once the scheme - and the fit of -em - has run, under
the parameters of -O PD.  PREFIXposteriorsampleSUFFIX holds one line per draw in the line format of the sequences file, whose
runs sum to T and are the runs of Chain.posterior_sample's paths for the chain of the same seed after the same scheme and fit;
PREFIXposteriorsamplesummarySUFFIX its header, a line per draw and, with -regions, a line per region."""
import os

import numpy as np
import pytest

from tests.cli_util import run_cli
from tests import oracle_lib as ol

pytestmark = pytest.mark.gpu
T, K, SEED = 20000, 3, 1
FLAGS = "-s %d -R %d -i F 30 1" % (K, SEED)


def fitted_chain(hml, x):
    g = hml.Chain(device=0, seed=SEED)
    g.load(x)
    g.set_model(K, g.autoprior(0.2, 0.9))
    g.sample_prior()
    g.iterate("F", 30, 1)
    g.sync()
    g.em_fit(5)
    return g


def runs_line(path, starts):
    out, b0 = [], 0
    for b in range(1, len(path) + 1):
        if b == len(path) or path[b] != path[b0]:
            out.append("%d:%d" % (starts[b] - starts[b0], path[b0]))
            b0 = b
    return "\t".join(out)


def test_sample_files_equal_the_chain(hml, tmp_path):
    x = ol.trace(T, K, 7)
    regions = str(tmp_path / "regions.txt")
    with open(regions, "w") as f:
        f.write("0 %d all\n100 101\n%d %d mid\n" % (T, T // 4, 3 * T // 4))
    r = run_cli(str(tmp_path), x, FLAGS + " -em 5 -psample 64 7 -regions " + regions, ["PS", "PSS", "PR"])
    assert r.returncode == 0, r.stderr
    g = fitted_chain(hml, x)
    s = g.posterior_sample(64, seed=7, paths=True)
    starts = g.blocks()
    lines = open(str(tmp_path / "g-posteriorsample.csv")).read().splitlines()
    assert len(lines) == 64
    for k, line in enumerate(lines):
        assert sum(int(t.split(":")[0]) for t in line.split("\t")) == T, k
        assert line == runs_line(s["paths"][k], starts), k
    lines = open(str(tmp_path / "g-posteriorsamplesummary.csv")).read().splitlines()
    assert len(lines) == 1 + 64 + 3
    head = lines[0].split("\t")
    assert head[:2] == ["64", "7"] and head[2] == "%.17g" % g.viterbi()[2][1] and head[3] == "%.17g" % g.posterior_breaks(2.0)["expected_breaks"]
    for k in range(64):
        assert lines[1 + k] == "%d\t%d\t%.17g" % (k, s["segments"][k], float(s["score_fixed"][k]) / 1048576.0), k
    start, end = np.array([0, 100, T // 4], np.uint32), np.array([T, 101, 3 * T // 4], np.uint32)
    reg = g.posterior_sample_regions(start, end, 64, seed=7, max_breaks=8)
    for i, label in enumerate(["all", "", "mid"]):
        want = ["%d" % start[i], "%d" % end[i], "%.17g" % (float(reg["breaks_sum"][i]) / 64.0)] + ["%d" % v for v in reg["hist"][i]] + [label]
        assert lines[65 + i].split("\t") == want, i
    assert reg["hist"][1, 0] == 64                                   # one position: no breakpoint inside
    assert os.path.exists(str(tmp_path / "g-posteriorregions.csv"))  # (stays as it is)


def test_seed_defaults_to_the_runs(hml, tmp_path):
    x = ol.trace(T, K, 7)
    r = run_cli(str(tmp_path), x, FLAGS + " -psample 3", ["PSS"])
    assert r.returncode == 0, r.stderr
    assert open(str(tmp_path / "g-posteriorsamplesummary.csv")).readline().split("\t")[:2] == ["3", str(SEED)]


def test_refusals(tmp_path):
    x = ol.trace(2000, K, 7)
    r = run_cli(str(tmp_path), x, "-s %d -R %d -i M 4 0 -psample 5" % (K, SEED), ["PS"])
    assert r.returncode == 1 and "need a model with transitions: the scheme has mixture sweeps only!" in r.stderr and "posteriorsample (PS)" in r.stderr
    r = run_cli(str(tmp_path), x, FLAGS, ["PSS"])
    assert r.returncode == 1 and "need the draws: ask for them with -psample R [SEED]!" in r.stderr
    r = run_cli(str(tmp_path), x, FLAGS + " -psample 0", ["PS"])
    assert r.returncode == 1 and "The first argument of -psample must be a whole number of draws" in r.stderr
    r = run_cli(str(tmp_path), x, FLAGS + " -psample 4 1 2", ["PS"])
    assert r.returncode == 1 and "Too many arguments for flag -psample" in r.stderr
    assert not os.path.exists(str(tmp_path / "g-posteriorsample.csv"))

"""`hammlet -O PB -pbreak P` and `-O PR -regions FILE` (extensions): PREFIXposteriorbreaksSUFFIX and
PREFIXposteriorregionsSUFFIX are written once the scheme (and a fit, with -em) has run, under the parameters of -O PD; parsed,
they hold what Chain.posterior_breaks and Chain.posterior_regions give for the chain of the same seed after the same scheme.
The shape is the baseline's config 1."""
import os

import numpy as np
import pytest

from tests.cli_util import run_cli
from tests import oracle_lib as ol

pytestmark = pytest.mark.gpu
T, K, SEED = 100000, 3, 1
FLAGS = "-s %d -R %d -i F 100 1" % (K, SEED)
REGIONS = [(0, T, "everything"), (0, 1, ""), (40000, 40500, "gene A"), (40000, 40500, "gene A again"), (99999, T, "last"), (123, 70000, "long one")]


def regions_file(tmp):
    fn = os.path.join(tmp, "regions.txt")
    with open(fn, "w") as f:
        f.write("# start end label\n")
        for a, e, label in REGIONS:
            f.write("%d %d %s\n" % (a, e, label))
    return fn


@pytest.mark.parametrize("fit", [False, True])
def test_the_two_files_hold_the_chain_s_words(hml, tmp_path, fit):
    x = ol.trace(T, K, 7)
    tmp = str(tmp_path)
    r = run_cli(tmp, x, FLAGS + " -pbreak 0.25 -regions " + regions_file(tmp) + (" -em 5" if fit else ""), ["PB", "PR", "PD"])
    assert r.returncode == 0, r.stderr
    g = hml.Chain(device=0, seed=SEED)
    g.load(x)
    g.set_model(K, g.autoprior(0.2, 0.9))
    g.sample_prior()
    g.iterate("F", 100, 1)
    g.sync()
    if fit:
        g.em_fit(5)
    b = g.posterior_breaks(0.25)
    lines = open(os.path.join(tmp, "g-posteriorbreaks.csv")).read().splitlines()
    assert lines[0] == "%.17g\t%d\t%.17g" % (b["expected_breaks"], b["pair_degenerate"], 0.25)
    assert lines[1:] == ["%d\t%.17g" % (p, v) for p, v in zip(b["pos"].tolist(), b["prob"].tolist())] and len(lines) > 1
    n = g.posterior_regions([a for a, _, _ in REGIONS], [e for _, e, _ in REGIONS])
    lines = open(os.path.join(tmp, "g-posteriorregions.csv")).read().splitlines()
    assert len(lines) == len(REGIONS)
    for i, (a, e, label) in enumerate(REGIONS):
        fields = lines[i].split("\t")
        assert fields[:2] == [str(a), str(e)] and fields[-1] == label and len(fields) == 5 + 2 * K, i
        want = [n["whole"][i], n["expected_breaks"][i]] + n["whole_state"][i].tolist() + n["share"][i].tolist()
        assert fields[2:-1] == ["%.17g" % v for v in want], i
        assert [float(v) for v in fields[2:-1]] == want, i       # (%.17g gives the double back)
    # the same parameters as the posterior file's
    assert open(os.path.join(tmp, "g-posterior.csv")).readline().split("\t")[0] == "%.17g" % g.posterior()[1]


def test_the_default_probability_is_a_half(hml, tmp_path):
    x = ol.trace(20000, K, 7)
    r = run_cli(str(tmp_path), x, "-s %d -R %d -i F 20 1" % (K, SEED), ["PB"])
    assert r.returncode == 0, r.stderr
    lines = open(str(tmp_path / "g-posteriorbreaks.csv")).read().splitlines()
    assert lines[0].split("\t")[2] == "0.5" and all(float(l.split("\t")[1]) >= 0.5 for l in lines[1:])


def test_refusals(tmp_path):
    x = ol.trace(2000, K, 7)
    tmp = str(tmp_path)
    r = run_cli(tmp, x, "-s %d -R %d -i M 4 0" % (K, SEED), ["PB"])
    assert r.returncode == 1 and "[ERROR] The outputs posteriorbreaks (PB) and posteriorregions (PR) need a model with transitions: the scheme has mixture sweeps only!" in r.stderr
    r = run_cli(tmp, x, "-s %d -R %d -i F 4 0" % (K, SEED), ["PR"])
    assert r.returncode == 1 and "[ERROR] The output posteriorregions (PR) needs the regions" in r.stderr
    r = run_cli(tmp, x, "-s %d -R %d -i F 4 0 -pbreak nan" % (K, SEED), ["PB"])
    assert r.returncode == 1 and "[ERROR] Conversion failed for string \"nan\"!" in r.stderr
    assert not os.path.exists(os.path.join(tmp, "g-posteriorbreaks.csv")) and not os.path.exists(os.path.join(tmp, "g-posteriorregions.csv"))

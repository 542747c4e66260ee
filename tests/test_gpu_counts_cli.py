"""`hammlet -O PC -regions FILE [-pcounts H]` (extension): PREFIXposteriorcountsSUFFIX is written once the scheme (and a fit,
with -em) has run, under the parameters of -O PD; parsed, it holds what Chain.posterior_region_counts gives for the chain of
the same seed after the same scheme - %.17g gives the doubles back."""
import os

import pytest

from tests.cli_util import CLI, run_cli
from tests import oracle_lib as ol

pytestmark = pytest.mark.gpu
T, K, SEED = 20000, 3, 1
FLAGS = "-s %d -R %d -i F 30 1" % (K, SEED)
REGIONS = [(0, T, "everything"), (0, 1, ""), (4000, 4500, "gene A"), (4000, 4500, "gene A again"), (T - 1, T, "last"), (123, 17000, "long one")]


def regions_file(tmp):
    fn = os.path.join(tmp, "regions.txt")
    with open(fn, "w") as f:
        f.write("# start end label\n")
        for a, e, label in REGIONS:
            f.write("%d %d %s\n" % (a, e, label))
    return fn


@pytest.mark.parametrize("fit,H", [(False, None), (True, 3)])
def test_the_file_holds_the_chain_s_words(hml, tmp_path, fit, H):
    x = ol.trace(T, K, 7)
    tmp = str(tmp_path)
    flags = FLAGS + " -regions " + regions_file(tmp) + (" -em 5" if fit else "") + (" -pcounts %d" % H if H else "")
    r = run_cli(tmp, x, flags, ["PC", "PD"])
    assert r.returncode == 0, r.stderr
    H = H or 8                                  # the default
    g = hml.Chain(device=0, seed=SEED)
    g.load(x)
    g.set_model(K, g.autoprior(0.2, 0.9))
    g.sample_prior()
    g.iterate("F", 30, 1)
    g.sync()
    if fit:
        g.em_fit(5)
    n = g.posterior_region_counts([a for a, _, _ in REGIONS], [e for _, e, _ in REGIONS], H)
    lines = open(os.path.join(tmp, "g-posteriorcounts.csv")).read().splitlines()
    assert len(lines) == len(REGIONS)
    for i, (a, e, _) in enumerate(REGIONS):
        fields = lines[i].split("\t")
        assert fields[:2] == [str(a), str(e)] and len(fields) == 2 + (H + 1) + K, i
        want = n["hist"][i].tolist() + n["avoid"][i].tolist()
        assert fields[2:] == ["%.17g" % v for v in want], i
        assert [float(v) for v in fields[2:]] == want, i       # (%.17g gives the double back)
    # the same parameters as the posterior file's
    assert open(os.path.join(tmp, "g-posterior.csv")).readline().split("\t")[0] == "%.17g" % g.posterior()[1]


def test_refusals(tmp_path):
    x = ol.trace(2000, K, 7)
    tmp = str(tmp_path)
    regions = regions_file(tmp).replace("regions.txt", "small.txt")
    with open(regions, "w") as f:
        f.write("0 10\n")
    r = run_cli(tmp, x, "-s %d -R %d -i F 4 0" % (K, SEED), ["PC"])
    assert r.returncode == 1 and "[ERROR] The output posteriorcounts (PC) needs the regions: give them with -regions FILE!" in r.stderr
    r = run_cli(tmp, x, "-s %d -R %d -i M 4 0 -regions %s" % (K, SEED, regions), ["PC"])
    assert r.returncode == 1 and "[ERROR] The output posteriorcounts (PC) needs a model with transitions: the scheme has mixture sweeps only!" in r.stderr
    for bad in ("0", "33", "2.5"):
        r = run_cli(tmp, x, "-s %d -R %d -i F 4 0 -regions %s -pcounts %s" % (K, SEED, regions, bad), ["PC"])
        assert r.returncode == 1 and "[ERROR] The argument of -pcounts must be a whole number of breakpoints, 1 to 32" in r.stderr, bad
    r = run_cli(tmp, x, "-s 64 -R %d -i F 4 0 -regions %s -pcounts 16" % (SEED, regions), ["PC"])
    assert r.returncode == 1 and "at most 1024" in r.stderr
    r = run_cli(tmp, x, "-s %d -R %d -i F 4 0 -regions %s -pcounts nan" % (K, SEED, regions), ["PC"])
    assert r.returncode == 1 and "[ERROR] Conversion failed for string \"nan\"!" in r.stderr
    assert not os.path.exists(os.path.join(tmp, "g-posteriorcounts.csv"))


def test_the_help_names_the_flag_and_the_output():
    import subprocess
    r = subprocess.run([CLI, "-h"], capture_output=True, text=True)
    assert r.returncode == 0 and "-pcounts H" in r.stdout and "posteriorcounts" in r.stdout and " PC " in r.stdout

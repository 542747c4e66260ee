"""`hammlet -regions FILE [-bands E0 ...] -O RG` (extensions; long form regions): PREFIXregionsSUFFIX against
tests/regions_util.py on the CPU checker's chain.  The file prints means and standard deviations as the levels file does -
double arithmetic, ONE rounding to float, %.9g, which gives the float back - so what it holds is compared as follows:
  integers (start, end, N, whole, the band columns), labels and order: exactly;
  mean and spread of the breakpoint count: exactly (sums of integers: numpy does the same double operations);
  the mean of the region's mean level: |file - reference| <= bound_sum / N + 2^-24 |reference|, the bound of
    tests/regions_util.py on the sum and the one rounding to float;
  its spread sd = sqrt(v), v = S2 / N - (S1 / N)^2: dv = bound_sq / N + 2 |mean| bound_sum / N + (bound_sum / N)^2 + 2^-50 (S2 / N)
    (the sums' bounds and the three double roundings of the formula), and since |sqrt(a) - sqrt(b)| equals |a - b| / (sqrt(a) +
    sqrt(b)) and never exceeds sqrt(|a - b|): |file - reference| <= min(sqrt(dv), dv / sd) + 2^-24 sd."""
import os
import subprocess

import numpy as np
import pytest

from tests import bands_cases as bc
from tests.cli_util import CLI, run_cli
from tests import oracle_lib as ol
from tests import regions_util as ru

pytestmark = pytest.mark.gpu
T, K, SEED = 50000, 3, 4
SCHEME = [("F", 20, 0), ("F", 30, 2)]
FLAGS = "-s %d -R %d -i F 20 0 F 30 2" % (K, SEED)
EDGES = (-0.5, 0.5)


def checker_sweeps(x, chain=0):
    c = dict(T=T, K=K, seed=SEED, scheme=SCHEME, trace=x, D=1, P=None, compat=False, env={})
    o = bc.checker(c, chain=chain)
    try:
        return bc.checker_sweeps(o, SCHEME)
    finally:
        o.close()


def regions_file(tmp, sweeps):
    start, end = ru.standard_regions(T, sweeps[-1], seed=7, n_random=200)
    labels = ["" if r % 3 == 0 else "gene%d exon %d" % (r, r % 5) for r in range(len(start))]
    fn = os.path.join(tmp, "regions.txt")
    with open(fn, "w") as f:
        f.write(ru.regions_file_text(start, end, labels))
    return fn, start, end, labels


def assert_file(text, want, start, end, labels, edges):
    ncol = len(edges) + 1 if len(edges) else 0
    got = ru.parse_output(text, 1, ncol)
    N = want["N"]
    assert list(got["start"]) == list(start) and list(got["end"]) == list(end) and got["label"] == labels      # file order kept
    assert np.all(got["N"] == N) and np.array_equal(got["whole"], want["whole"].astype(np.int64))
    assert np.array_equal(got["inband"], want["inband"].astype(np.int64))
    bmean = want["breaks_sum"].astype(np.float64) / N
    bsd = np.sqrt(np.maximum(want["breaks_sq"].astype(np.float64) / N - bmean * bmean, 0.0))
    assert np.array_equal(got["breaks_mean"].astype(np.float32), bmean.astype(np.float32))
    assert np.array_equal(got["breaks_sd"].astype(np.float32), bsd.astype(np.float32))
    mean = (want["level_sum"][0] / N).astype(np.float64)
    s2 = (want["level_sq"][0] / N).astype(np.float64)
    sd = np.sqrt(np.maximum((want["level_sq"][0] / N - (want["level_sum"][0] / N) ** 2).astype(np.float64), 0.0))
    d_mean = want["bound_sum"] / N
    tol_mean = d_mean + 2.0 ** -24 * np.abs(mean)
    dv = want["bound_sq"] / N + 2 * np.abs(mean) * d_mean + d_mean ** 2 + 2.0 ** -50 * s2
    with np.errstate(divide="ignore"):
        tol_sd = np.minimum(np.sqrt(dv), np.where(sd > 0, dv / sd, np.inf)) + 2.0 ** -24 * sd
    err_mean, err_sd = np.abs(got["level_mean"][0] - mean), np.abs(got["level_sd"][0] - sd)
    print("largest error of the mean %.3e (tolerance there %.3e), of the spread %.3e (%.3e)" %
          (err_mean.max(), tol_mean[np.argmax(err_mean)], err_sd.max(), tol_sd[np.argmax(err_sd)]))
    assert np.all(err_mean <= tol_mean) and np.all(err_sd <= tol_sd)
    return got


@pytest.mark.parametrize("bands", [True, False])
def test_cli_regions_file(tmp_path, bands):
    """-O RG with and without -bands: without the edges the file has no band columns"""
    x = ol.trace(T, K, 1)
    sweeps = checker_sweeps(x)
    fn, start, end, labels = regions_file(str(tmp_path), sweeps)
    edges = EDGES if bands else ()
    r = run_cli(str(tmp_path), x, FLAGS + " -regions " + fn + (" -bands -0.5 0.5" if bands else ""), ["RG"])
    assert r.returncode == 0, r.stderr
    want = ru.accumulate(sweeps, start, end, edges)
    assert want["N"] == 15 and np.any(want["whole"] == 15) and np.any(want["whole"] < 15) and want["breaks_sum"].max() > 1
    got = assert_file(open(str(tmp_path / "g-regions.csv")).read(), want, start, end, labels, edges)
    assert got["inband"].shape == (len(start), 3 if bands else 0)
    assert sorted(f for f in os.listdir(str(tmp_path)) if f.startswith("g-")) == ["g-regions.csv"]


def test_cli_regions_three_chains_on_one_gpu(tmp_path):
    """`-chains 3` on one GPU: the chains' sums are added into the first chain's before the file is written (N = 45)"""
    x = ol.trace(T, K, 1)
    sweeps = []
    for k in range(3):
        sweeps += checker_sweeps(x, chain=k)
    fn, start, end, labels = regions_file(str(tmp_path), sweeps[:15])
    r = run_cli(str(tmp_path), x, "-chains 3 -bands -0.5 0.5 -regions " + fn + " " + FLAGS, ["regions"], one_gpu=True)
    assert r.returncode == 0, r.stderr
    want = ru.accumulate(sweeps, start, end, EDGES)
    assert want["N"] == 45
    assert_file(open(str(tmp_path / "g-regions.csv")).read(), want, start, end, labels, EDGES)


@pytest.mark.parametrize("text,message", ru.MALFORMED)
def test_cli_regions_refusals(tmp_path, text, message):
    raw = str(tmp_path / "in.f32")
    ol.trace(2000, K, 1).tofile(raw)
    fn = ru.write_malformed(str(tmp_path), text)
    r = subprocess.run([CLI, "-raw", raw, "-o", str(tmp_path / "g-"), ".csv", "-a", "-w"] + FLAGS.split() + ["-bands", "-0.5", "0.5", "-regions", fn, "-O", "RG", "M"],
                       capture_output=True, text=True)
    assert r.returncode == 1 and message in r.stderr, r.stderr
    assert [f for f in os.listdir(str(tmp_path)) if f.startswith("g-")] == []


def test_cli_other_files_unchanged_by_the_regions(tmp_path):
    """a run without the new flags writes what it writes with them, byte for byte, and no regions file"""
    x = ol.trace(T, K, 1)
    fn, start, end, labels = regions_file(str(tmp_path), [(np.array([0, T // 2, T]),)])
    outs = ["M", "P", "L", "BP"]
    r0 = run_cli(str(tmp_path), x, FLAGS, outs, prefix="a-")
    r1 = run_cli(str(tmp_path), x, FLAGS + " -regions " + fn, outs + ["RG"], prefix="b-")
    assert r0.returncode == 0 and r1.returncode == 0, (r0.stderr, r1.stderr)
    for name in ("marginals", "parameters", "levels", "breakpoints"):
        a = open(str(tmp_path / ("a-%s.csv" % name)), "rb").read()
        assert len(a) > 0 and a == open(str(tmp_path / ("b-%s.csv" % name)), "rb").read(), name
    assert not os.path.exists(str(tmp_path / "a-regions.csv")) and os.path.exists(str(tmp_path / "b-regions.csv"))

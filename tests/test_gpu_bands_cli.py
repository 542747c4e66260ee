"""`hammlet -bands E0 [E1 ...] -O LB LC` (extensions; long forms bands and bandcalls): PREFIXbandsSUFFIX and
PREFIXbandcallsSUFFIX against text written from tests/bands_util.py on the CPU checker's chain."""
import os

import numpy as np
import pytest

from tests import bands_cases as bc
from tests import bands_util as bu
from tests.cli_util import run_cli
from tests import oracle_lib as ol

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


def expected_texts(sweeps, p):
    counts, boundary, N = bu.accumulate(sweeps, T, EDGES)
    length, seg = bu.rle(counts, boundary)
    return bu.bands_text(length, seg), bu.calls_text(*bu.call(seg, length, bu.rank_of(p, N), 1, len(EDGES) + 1)), N


@pytest.mark.parametrize("bandcall", [None, "0.5"])
def test_cli_bands_and_bandcalls_files(tmp_path, bandcall):
    x = ol.trace(T, K, 1)
    r = run_cli(str(tmp_path), x, FLAGS + " -bands -0.5 0.5" + (" -bandcall " + bandcall if bandcall else ""), ["LB", "LC"])
    assert r.returncode == 0, r.stderr
    bands, calls, N = expected_texts(checker_sweeps(x), float(bandcall or 0))
    assert N == 15 and len(bands.splitlines()) > 1 and len(calls.splitlines()) > 1
    assert open(str(tmp_path / "g-bands.csv")).read() == bands
    assert open(str(tmp_path / "g-bandcalls.csv")).read() == calls
    assert not os.path.exists(str(tmp_path / "g-marginals.csv"))


def test_cli_bands_three_chains_on_one_gpu(tmp_path):
    """`-chains 3` on one GPU: the chains' counts are merged into the first before the files are written"""
    x = ol.trace(T, K, 1)
    r = run_cli(str(tmp_path), x, "-chains 3 -bands -0.5 0.5 " + FLAGS, ["bands", "bandcalls"], one_gpu=True)
    assert r.returncode == 0, r.stderr
    sweeps = []
    for k in range(3):
        sweeps += checker_sweeps(x, chain=k)
    bands, calls, N = expected_texts(sweeps, 0)
    assert N == 45
    assert open(str(tmp_path / "g-bands.csv")).read() == bands
    assert open(str(tmp_path / "g-bandcalls.csv")).read() == calls


@pytest.mark.parametrize("flags,outputs,message", [
    ("", ["LB"], "need the edges of the bands"),
    ("", ["LC"], "need the edges of the bands"),
    ("-bands 0.5 -0.5", ["LB"], "must be strictly ascending"),
    ("-bands 0.5 0.5", ["LB"], "must be strictly ascending"),
    ("-bands 0 inf", ["LB"], "must be finite"),
    ("-bands " + " ".join(str(j) for j in range(32)), ["LB"], "at most 31"),
    ("-bands -0.5 0.5 -bandcall 1.5", ["LC"], "must lie in [0, 1]"),
])
def test_cli_bands_refusals(tmp_path, flags, outputs, message):
    x = ol.trace(2000, K, 1)
    r = run_cli(str(tmp_path), x, FLAGS + " " + flags, outputs)
    assert r.returncode == 1 and message in r.stderr, r.stderr
    assert not os.path.exists(str(tmp_path / "g-bands.csv")) and not os.path.exists(str(tmp_path / "g-bandcalls.csv"))


def test_cli_other_files_unchanged_by_the_new_flags(tmp_path):
    """a run without the new flags writes what it writes with them, byte for byte, and no band file"""
    x = ol.trace(T, K, 1)
    outs = ["M", "P", "X", "L", "BP"]
    r0 = run_cli(str(tmp_path), x, FLAGS, outs, prefix="a-")
    r1 = run_cli(str(tmp_path), x, FLAGS + " -bands -0.5 0.5", outs + ["LB", "LC"], prefix="b-")
    assert r0.returncode == 0 and r1.returncode == 0, (r0.stderr, r1.stderr)
    for name in ("marginals", "parameters", "maxsegmentation", "levels", "breakpoints"):
        a = open(str(tmp_path / ("a-%s.csv" % name)), "rb").read()
        assert len(a) > 0 and a == open(str(tmp_path / ("b-%s.csv" % name)), "rb").read(), name
    assert sorted(f for f in os.listdir(str(tmp_path)) if f.startswith("a-")) == sorted("a-%s.csv" % n for n in ("marginals", "parameters", "maxsegmentation", "levels", "breakpoints"))
    assert os.path.exists(str(tmp_path / "b-bands.csv")) and os.path.exists(str(tmp_path / "b-bandcalls.csv"))

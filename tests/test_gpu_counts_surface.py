"""hammlet::Posterior::regionCounts, ::countsInfo and ::writeCountsFile (include/hammlet/Posterior.hpp) from C++:
tests/fixtures/counts_surface_main.cpp calls them on a chain of its own and prints every double as its word; the chain of the
same seed in Python gives the same words, and the file holds them as %.17g, which gives the doubles back."""
import os
import subprocess

import numpy as np
import pytest

from tests import oracle_lib as ol
from tests import posterior_util as pu

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "fixtures", "counts_surface_main.cpp")
T, K, SEED, H = 20000, 3, 9, 5


def test_region_counts_from_cpp(hml, tmp_path):
    exe = str(tmp_path / "counts_surface")
    lib = os.path.join(REPO, "hammlet_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), "-o", exe, SRC, "-L", lib, "-lhammlet_hip",
                    "-Wl,-rpath," + lib], check=True)
    x = ol.trace(T, K, 23)
    raw, out = str(tmp_path / "in.f32"), str(tmp_path / "counts.csv")
    x.tofile(raw)
    r = subprocess.run([exe, raw, str(K), str(SEED), str(H), out], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    got = {}
    for line in r.stdout.splitlines():
        name, _, rest = line.partition(" ")
        got[name] = rest.split()
    g = hml.Chain(device=0, seed=SEED)
    g.load(x)
    g.set_model(K, g.autoprior(0.2, 0.9))
    g.sample_prior()
    g.iterate("F", 3, 0)
    g.sync()
    hexes = lambda a: ["%x" % v for v in pu.words(a).tolist()]
    start, end = np.array(got["start"], np.uint32), np.array(got["end"], np.uint32)
    assert start.tolist() == [0, 0, T // 4, 100, T // 2] and end.tolist() == [T, 1, 3 * (T // 4), 101, T // 2 + 1000]
    n = g.posterior_region_counts(start, end, H)
    for key in ("hist", "whole_state", "avoid"):
        assert got[key] == hexes(n[key]), key
    assert got["degenerate"] == [str(n["count_degenerate"])]
    info = g.posterior_counts_info()
    assert got["info"] == [str(info[k]) for k in ("regions", "steps", "longest")] and info["regions"] == 5 and info["longest"] > 0
    lines = open(out).read().splitlines()
    assert len(lines) == 5
    for i, line in enumerate(lines):
        fields = line.split("\t")
        want = n["hist"][i].tolist() + n["avoid"][i].tolist()
        assert fields[:2] == [str(start[i]), str(end[i])] and len(fields) == 2 + (H + 1) + K, i
        assert fields[2:] == ["%.17g" % v for v in want] and [float(v) for v in fields[2:]] == want, i
    # a max_breaks outside the rule reaches the caller as the library's message
    bad = subprocess.run([exe, raw, str(K), str(SEED), "33", out], capture_output=True, text=True)
    assert bad.returncode == 1 and "max_breaks must be 1 ... 32" in bad.stderr

"""hammlet::Posterior::breaks and ::regions (include/hammlet/Posterior.hpp) from C++: tests/fixtures/pairs_surface_main.cpp
calls them on a chain of its own and prints every double as its word; the chain of the same seed in Python gives the same
words."""
import os
import subprocess

import numpy as np
import pytest

from tests import oracle_lib as ol
from tests import posterior_util as pu

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "fixtures", "pairs_surface_main.cpp")
T, K, SEED, MIN_PROB = 20000, 3, 9, 0.25


def test_breaks_and_regions_from_cpp(hml, tmp_path):
    exe = str(tmp_path / "pairs_surface")
    lib = os.path.join(REPO, "hammlet_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), "-o", exe, SRC, "-L", lib, "-lhammlet_hip",
                    "-Wl,-rpath," + lib], check=True)
    x = ol.trace(T, K, 23)
    raw = str(tmp_path / "in.f32")
    x.tofile(raw)
    r = subprocess.run([exe, raw, str(K), str(SEED), repr(MIN_PROB)], capture_output=True, text=True)
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
    b = g.posterior_breaks(MIN_PROB)
    assert got["pos"] == [str(v) for v in b["pos"].tolist()] and got["prob"] == hexes(b["prob"])
    assert got["breaks"] == hexes([b["expected_breaks"]]) + [str(b["pair_degenerate"])]
    start, end = np.array(got["start"], np.uint32), np.array(got["end"], np.uint32)
    assert start.tolist() == [0, 0, T // 4, 100, T // 2] and end.tolist() == [T, 1, 3 * (T // 4), 101, T // 2 + 1000]
    n = g.posterior_regions(start, end)
    for key in ("whole", "whole_state", "expected_breaks", "share"):
        assert got[key] == hexes(n[key]), key
    assert got["degenerate"] == [str(n["pair_degenerate"])]
    assert 0 < len(b["pos"]) < g.num_blocks() - 1

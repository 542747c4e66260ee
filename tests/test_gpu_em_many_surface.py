"""hammlet::Fit::starts, fitMany and writeStartsFile (include/hammlet/Fit.hpp) from C++: tests/fixtures/fit_many_surface_main.cpp
runs a batch on a chain of its own and prints every double and float as its word; the chain of the same seed in Python gives
the same words."""
import os
import subprocess

import pytest

from tests import oracle_lib as ol
from tests import posterior_util as pu

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "fixtures", "fit_many_surface_main.cpp")
T, K, SEED, R, STARTS_SEED, STEPS = 20000, 3, 9, 4, 11, 4
REASON = {0: "max_steps", 1: "converged", 2: "degenerate"}


def test_fit_many_from_cpp(hml, tmp_path):
    exe = str(tmp_path / "fit_many_surface")
    lib = os.path.join(REPO, "hammlet_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), "-o", exe, SRC, "-L", lib, "-lhammlet_hip",
                    "-Wl,-rpath," + lib], check=True)
    x = ol.trace(T, K, 23)
    raw, out = str(tmp_path / "in.f32"), str(tmp_path / "starts.csv")
    x.tofile(raw)
    r = subprocess.run([exe, raw, str(K), str(SEED), str(R), str(STARTS_SEED), str(STEPS), out], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines()]
    g = hml.Chain(device=0, seed=SEED)
    g.load(x)
    g.set_model(K, g.autoprior(0.2, 0.9))
    g.sample_prior()
    g.iterate("F", 3, 0)
    g.sync()
    starts = g.em_starts(R, STARTS_SEED)
    got = g.em_fit_many(starts=starts, max_steps=STEPS)
    hexes = lambda a: ["%x" % v for v in pu.words(a).tolist()]
    hexes32 = lambda a: ["%x" % v for v in pu.words32(a).ravel().tolist()]
    assert lines[0] == ["starts"] + hexes32(starts[0])
    for m in range(R):
        n = int(got["steps"][m])
        assert lines[1 + 3 * m] == ["trace"] + hexes(got["trace"][m][:n + 1]), m
        assert lines[2 + 3 * m] == ["member", str(n), REASON[int(got["reason"][m])], str(got["kept"][m])], m
        assert lines[3 + 3 * m] == ["mean_var"] + hexes32(got["mean_var"][m]), m
    assert lines[1 + 3 * R] == ["best", str(got["best"])] and got["best"] >= 0
    assert lines[2 + 3 * R] == ["installed"] + hexes32(g.theta()) == ["installed"] + hexes32(got["mean_var"][got["best"]])
    rows = open(out).read().splitlines()
    assert len(rows) == R and [row.endswith("\t*") for row in rows] == [m == got["best"] for m in range(R)]
    assert rows[1].split("\t")[:5] == ["1", "%.17g" % got["objective"][1], str(got["steps"][1]), REASON[int(got["reason"][1])], str(got["kept"][1])]

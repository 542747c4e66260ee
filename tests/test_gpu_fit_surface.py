"""hammlet::Fit (include/hammlet/Fit.hpp) from C++: tests/fixtures/fit_surface_main.cpp calls expectedCounts(), step() and
fit() on a chain of its own and prints every double as its word; the chain of the same seed in Python gives the same words."""
import os
import subprocess

import numpy as np
import pytest

from tests import oracle_lib as ol
from tests import posterior_util as pu

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "fixtures", "fit_surface_main.cpp")
T, K, SEED = 20000, 3, 9


def test_fit_from_cpp(hml, tmp_path):
    exe = str(tmp_path / "fit_surface")
    lib = os.path.join(REPO, "hammlet_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), "-o", exe, SRC, "-L", lib, "-lhammlet_hip",
                    "-Wl,-rpath," + lib], check=True)
    x = ol.trace(T, K, 23)
    raw = str(tmp_path / "in.f32")
    x.tofile(raw)
    r = subprocess.run([exe, raw, str(K), str(SEED)], capture_output=True, text=True)
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
    n = g.expected_counts()
    hexes = lambda a: ["%x" % v for v in pu.words(a).tolist()]
    for key in ("xi", "first", "stay", "occ", "sum", "sum_sq"):
        assert got[key] == hexes(n[key]), key
    assert got["loglik"] == hexes([n["loglik"]]) and got["degenerate"] == [str(n["degenerate"]), str(n["xi_degenerate"])]
    objective, kept = g.em_step(use_prior=True)      # (with a prior exponent below 1 the objective may be +inf: words either way)
    assert got["step"] == hexes([objective]) + [str(kept)]
    trace, steps, reason, kept = g.em_fit(2, rel_tol=-1.0)
    assert got["trace"] == hexes(trace) and steps == 2 and reason == hml.EM_MAX_STEPS
    assert got["fit"] == [str(steps), "max_steps", str(kept)]
    assert np.isfinite(trace).all() and trace[2] >= trace[1]

"""hammlet::Posterior::sample and ::sampleRegions (include/hammlet/Posterior.hpp) from C++: tests/fixtures/sample_surface_main.cpp
calls them on a chain of its own and prints every word; the chain of the same seed in Python gives the same words."""
import os
import subprocess

import numpy as np
import pytest

from tests import oracle_lib as ol

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "fixtures", "sample_surface_main.cpp")
T, K, SEED, FIRST, COUNT, SAMPLE_SEED = 20000, 3, 9, 5, 70, 13


def test_sample_and_regions_from_cpp(hml, tmp_path):
    exe = str(tmp_path / "sample_surface")
    lib = os.path.join(REPO, "hammlet_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), "-o", exe, SRC, "-L", lib, "-lhammlet_hip",
                    "-Wl,-rpath," + lib], check=True)
    x = ol.trace(T, K, 23)
    raw = str(tmp_path / "in.f32")
    x.tofile(raw)
    r = subprocess.run([exe, raw, str(K), str(SEED), str(FIRST), str(COUNT), str(SAMPLE_SEED)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    got = {}
    for line in r.stdout.splitlines():
        name, _, rest = line.partition(" ")
        got[name] = np.array(rest.split(), np.int64)
    g = hml.Chain(device=0, seed=SEED)
    g.load(x)
    g.set_model(K, g.autoprior(0.2, 0.9))
    g.sample_prior()
    g.iterate("F", 3, 0)
    g.sync()
    s = g.posterior_sample(COUNT, seed=SAMPLE_SEED, first=FIRST, paths=True, state_counts=True)
    for key in ("paths", "segments", "score_fixed", "change_count", "state_count"):
        assert np.array_equal(got[key], np.asarray(s[key]).ravel().astype(np.int64)), key
    assert got["degenerate"][0] == s["sample_degenerate"]
    assert got["start"].tolist() == [0, 0, T // 4, 100, T // 2] and got["end"].tolist() == [T, 1, 3 * (T // 4), 101, T // 2 + 1000]
    n = g.posterior_sample_regions(got["start"], got["end"], COUNT, seed=SAMPLE_SEED, first=FIRST, max_breaks=3)
    for key in ("hist", "whole_state", "breaks_sum", "breaks_sq"):
        assert np.array_equal(got[key], n[key].ravel().astype(np.int64)), key
    starts, q = g.blocks().astype(np.int64), s["paths"][0]
    heads = np.flatnonzero(np.concatenate([[True], q[1:] != q[:-1]]))
    assert np.array_equal(got["run_state"], q[heads]) and np.array_equal(got["run_len"], np.diff(np.concatenate([starts[heads], [T]])))
    assert got["info"].tolist() == [COUNT, 1, COUNT] and len(heads) == s["segments"][0] and 1 < len(heads) < g.num_blocks()

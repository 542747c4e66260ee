"""Exact inference on the device (hml_infer.hip: Viterbi decode, smoothing, E-step and fit, EM from many starts, pairwise
read-outs, path sampler) on inputs that are not a unit-scale Gaussian trace, against the restatements for one host thread
(tests/fixtures/*_ref_main.cpp over hammlet_amd/csrc/hml_*_ref.h), which are fed the GPU's own block_stats(), blocks(), theta()
and transitions():
  (a) chains on the scale, offset, depth and spikes families of tests/hostile_inputs.py, five sweeps, the first 20 000 positions;
  (b) the planted cases of tests/infer_cases.py that a chain can reach, with the coverage flags of tests/test_infer_hostile_cpu.py
      asserted again from the programs' output for the GPU's statistics;
  (c) an all-degenerate and a partly degenerate case under geometries that make the repair rounds and the single lane run.
Every pass goes through the check functions of its own test module (tests/infer_fuzz_util.check_pass).  A word is the program's,
or - where that is the NaN the host makes - the NaN the device makes (tests/words_util.expected_words); any other NaN is a
difference.  Floats are compared as their 32-bit, doubles as their 64-bit words: there is no tolerance anywhere in this file.

Wall time of the module on one MI355X, measured once: 15 s for its 136 tests; the slowest - EM from three starts at 20 states -
0.9 s."""

import numpy as np
import pytest

from tests import hostile_inputs as hi
from tests import infer_cases as ic
from tests import pairs_util as pz
from tests import posterior_util as pu
from tests import sample_util as su
from tests import test_gpu_em as te
from tests import test_gpu_posterior as tpo
from tests import test_gpu_sample as ts
from tests import test_gpu_viterbi as tv
from tests.infer_fuzz_util import N_PATHS, NIG4, PASSES, build_programs, check_pass, device_nans

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    return build_programs(tmp_path_factory.mktemp("infer_hostile"))


# ---------------------------------------------------------------------------------------------- (a) hostile chains
HOSTILE = hi.family("scale", "offset", "depth", "spikes")


@pytest.mark.parametrize("pass_", PASSES)
@pytest.mark.parametrize("name", HOSTILE)
def test_chains_on_hostile_inputs(hml, programs, name, pass_):
    _, K, _ = hi.INPUTS[name]
    g = te.chain(hml, hi.data(name)[:20000], K, seed=hi.SEED[name], sweeps=5)
    with device_nans(g):
        check_pass(hml, programs, g, pass_, what=(name, pass_))
    g.close()


# ---------------------------------------------------------------------------------------------- (b) planted cases
def planted_chain(hml, name, T=None):
    """the recipe on the device: data loaded, every position a block, set_parameters (no automatic prior: it is the planted
    parameters that count)"""
    r = ic.CASES[name](T)
    assert r["block"] == 1
    g = hml.Chain(device=0, seed=3)
    if r["D"] > 1:
        g.set_dimensions(r["D"], r["P"])
    g.load(r["x"])
    g.em_nig4 = NIG4
    g.set_model(r["K"], NIG4, self_trans=r["self_trans"])
    g.sample_prior()
    g.create_blocks(0.0)                                  # `!(w < 0)`: every position starts a block
    g.set_parameters(r["mean_var"], r["A"], r["pi"])
    assert g.num_blocks() == g.T == r["x"].size // r["D"]
    return g, r


@pytest.mark.parametrize("name", ic.DEVICE)
def test_planted_cases(hml, programs, name):
    g, r = planted_chain(hml, name)
    seen = {}
    with device_nans(g):
        for pass_ in PASSES:
            seen.update(check_pass(hml, programs, g, pass_, r["self_trans"], (name, pass_)))
    held = ic.flags(pu.chain_case(g, r["self_trans"]), seen)
    assert ic.EXPECT[name] <= held, (name, sorted(ic.EXPECT[name] - held))
    g.close()


# ---------------------------------------------------------------------------------------------- (c) geometry
GEOMETRIES = [(1, 4, 0), (1, 64, 1), (4, 64, 8), (1024, 4, 8)]      # (W, L, rounds)
GEOMETRY_T = 1000


@pytest.mark.parametrize("name", ["all_degenerate", "var_denormal"])
def test_geometry_is_invisible_on_degenerate_blocks(hml, programs, name):
    g, r = planted_chain(hml, name, GEOMETRY_T)
    B = g.num_blocks()
    want_v = tv.reference(programs["viterbi"], g)
    with device_nans(g):
        want_p = tpo.reference(programs["posterior"], g)
    regions = pz.edge_regions(g.blocks(), np.random.default_rng(5), n_random=3)
    want_s = ts.reference(programs["sample"], g, N_PATHS, 7, regions=regions)
    assert want_p["degenerate"] == B if name == "all_degenerate" else 0 < want_p["degenerate"] < B
    for W, L, rounds in GEOMETRIES:
        geo = (name, W, L, rounds)
        for pass_ in ("viterbi", "posterior", "sample"):
            g.set_option(pass_ + "_W", W)
            g.set_option(pass_ + "_L", L)
            g.set_option(pass_ + "_rounds", rounds)
        chunks = (B + L - 1) // L
        tv.check_decode(g, want_v, geo)
        info = g.viterbi_info()
        assert info["W"] == W and info["L"] == L and info["chunks"] == chunks and info["rounds"] <= rounds, (geo, info)
        assert info["stale_chunks"] < info["chunks"] and info["serial_chunks"] <= info["chunks"] - 1, (geo, info)
        if info["stale_chunks"] == 0 or rounds == 0:
            assert info["rounds"] == 0, (geo, info)
        if info["stale_chunks"] == 0:
            assert info["serial_chunks"] == 0, (geo, info)
        tpo.check_results(g, want_p, geo)
        info = g.posterior_info()
        assert info["W"] == W and info["L"] == L and info["chunks"] == chunks and info["rounds"] <= rounds, (geo, info)
        assert info["stale_fwd"] < info["chunks"] and info["stale_bwd"] < info["chunks"] and info["serial_chunks"] <= 2 * (info["chunks"] - 1), (geo, info)
        if info["stale_fwd"] + info["stale_bwd"] == 0 or rounds == 0:
            assert info["rounds"] == 0, (geo, info)
        if info["stale_fwd"] + info["stale_bwd"] == 0:
            assert info["serial_chunks"] == 0, (geo, info)
        ts.check_sample(g, want_s, N_PATHS, 7, what=geo)
        reg = g.posterior_sample_regions(regions[0], regions[1], N_PATHS, seed=7, max_breaks=ts.H)
        su.same(reg, want_s, su.REGION_KEYS, geo)
        info = g.posterior_sample_info()
        assert info["W"] == W and info["L"] == L and info["chunks"] == chunks and info["rounds"] <= rounds, (geo, info)
        assert info["stale_first"] <= N_PATHS * (chunks - 1) and info["serial_chunks"] <= N_PATHS * (chunks - 1), (geo, info)
        if info["stale_first"] == 0 or rounds == 0:
            assert info["rounds"] == 0, (geo, info)
        if info["stale_first"] == 0:
            assert info["serial_chunks"] == 0, (geo, info)
    g.close()

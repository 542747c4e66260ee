"""`hammlet -chains N -O rhat` (extension): PREFIXrhatSUFFIX, the agreement of the N chains of one GPU on the emission level,
taken before the chains are merged - against the C ABI on the same chains, and the levels file of the same run against the run
without `-O rhat`."""
import os

import numpy as np
import pytest

from tests import cli_util
from tests import oracle_lib as ol

pytestmark = pytest.mark.gpu
T, K, SEED = 100000, 3, 4


def run_cli(tmp, x, flags, outputs, prefix="g-", overwrite=True):
    """the chains of these runs share the first GPU"""
    return cli_util.run_cli(tmp, x, flags, outputs, one_gpu=True, prefix=prefix, overwrite=overwrite)


def api_chain(hml, x, chain=0, attach=None):
    g = hml.Chain(device=0, seed=SEED, chain_id=chain)
    if attach is None:
        g.load(x)
    else:
        g.attach(attach)
    g.set_model(K, g.autoprior(0.2, 0.9))
    g.set_level_recording(True)
    g.sample_prior()
    return g


def test_cli_rhat_file_of_three_chains(hml, tmp_path):
    x = ol.trace(T, K, 1)
    flags = "-s %d -R %d -chains 3 -i F 40 2" % (K, SEED)
    r = run_cli(str(tmp_path), x, flags + " -v", ["rhat", "L"])
    assert r.returncode == 0, r.stderr
    text = open(str(tmp_path / "g-rhat.csv")).read()
    a = api_chain(hml, x, chain=0)
    chains = [a] + [api_chain(hml, x, chain=k, attach=a) for k in (1, 2)]
    hml.iterate_many(chains, "F", 40, 2)
    for g in chains:
        g.sync()
    seg, n, within, between, rhat = hml.levels_agreement_rle(chains)
    assert n == 20 and seg.sum() == T and len(seg) > 1
    want = "".join("%d %s\n" % (int(seg[i]), "%.9g" % rhat[0, i]) for i in range(len(seg)))
    assert text == want
    # -v: the positions above 1.1 and the largest finite value
    above, largest, infinite = hml.levels_agreement_summary(chains, 1.1)
    line = [l for l in r.stdout.splitlines() if l.startswith("Positions with R-hat above 1.1")]
    assert len(line) == 1 and line[0].split(":")[1].split(";")[0].split() == [str(int(above[0]))]
    # the merge order: the levels file is the one of the same run without -O rhat
    r2 = run_cli(str(tmp_path), x, flags, ["L"], prefix="h-")
    assert r2.returncode == 0, r2.stderr
    assert open(str(tmp_path / "g-levels.csv"), "rb").read() == open(str(tmp_path / "h-levels.csv"), "rb").read()
    assert not os.path.exists(str(tmp_path / "h-rhat.csv"))
    # an existing rhat file is refused without -w, before anything runs
    r3 = run_cli(str(tmp_path), x, flags, ["rhat"], overwrite=False)
    assert r3.returncode == 1 and "g-rhat.csv already exists" in r3.stderr
    assert open(str(tmp_path / "g-rhat.csv")).read() == text


def test_cli_rhat_needs_two_chains(tmp_path):
    x = ol.trace(T, K, 1)
    r = run_cli(str(tmp_path), x, "-s %d -R %d -chains 1 -i F 10 1" % (K, SEED), ["rhat"])
    assert r.returncode == 1 and "compares the chains of one run" in r.stderr and "-chains N" in r.stderr
    assert sorted(os.listdir(str(tmp_path))) == ["in.f32"]

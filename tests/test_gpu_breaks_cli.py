"""`hammlet -O breakpoints consensus` (extensions; short forms BP and CS - B and C are the reference's blocks and
compression): PREFIXbreakpointsSUFFIX and PREFIXconsensusSUFFIX against files written from tests/breaks_util.py on the CPU
checker's chain."""
import os

import numpy as np
import pytest

from tests import breaks_cases as bc
from tests import breaks_util as bu
from tests.cli_util import run_cli
from tests import levels_util as lu
from tests import oracle_lib as ol

pytestmark = pytest.mark.gpu
T, K, SEED = 100000, 3, 4
SCHEME = [("F", 20, 0), ("F", 30, 2)]
FLAGS = "-s %d -R %d -i F 20 0 F 30 2" % (K, SEED)


def checker_sweeps(x, chain=0):
    c = dict(T=T, K=K, seed=SEED, scheme=SCHEME, trace=x, D=1, P=None, compat=False, env={})
    o = bc.checker(c, chain=chain)
    try:
        return bc.checker_sweeps(o, SCHEME)
    finally:
        o.close()


def breakpoints_text(C, N):
    pos, cnt = bu.listing(C)
    return "".join("%d %d %.9g\n" % (p, c, float(c) / float(N)) for p, c in zip(pos, cnt))


def assert_consensus_file(path, sweeps, C, N, window, share):
    """start, length and support as text; mean and standard deviation within the float32 rounding of the file plus the
    arithmetic's bound on the segment sums (breaks_util.segment_bounds) carried through sum / (N length)"""
    (pos, mass, peak), _ = bu.consensus(C, window, bu.min_count_of(share, N))
    assert len(pos) > 0
    S1, S2, boundary, Nl = lu.accumulate(sweeps, T)
    want1, length = bu.segment_sums(S1, pos)
    want2, _ = bu.segment_sums(S2, pos)
    B1, B2 = bu.segment_bounds(int(boundary.sum()), Nl, lu.max_abs_mean(sweeps), T, length)
    rows = [line.split() for line in open(path).read().splitlines()]
    assert len(rows) == len(pos) + 1
    starts = np.concatenate([[0], pos])
    support = ["1"] + ["%.9g" % (float(m) / float(N)) for m in mass]
    for k, r in enumerate(rows):
        assert len(r) == 5
        assert (int(r[0]), int(r[1]), r[2]) == (int(starts[k]), int(length[k]), support[k]), k
        w = float(Nl) * float(length[k])
        mean = want1[0, k] / w
        var = max(0.0, want2[0, k] / w - mean * mean)
        mu_max = lu.max_abs_mean(sweeps)
        tol_mean = B1[k] / w + 2.0 ** -23 * abs(mean)
        # d var <= d(S2 / w) + 2 |mean| d mean; the root is taken of a value that may be near zero: compare the squares
        tol_var = B2[k] / w + 2.0 * mu_max * B1[k] / w
        assert abs(float(r[3]) - mean) <= tol_mean, (k, r[3], mean, tol_mean)
        sd = float(r[4])
        assert abs(sd * sd - var) <= tol_var + 2.0 ** -22 * max(var, sd * sd), (k, r[4], var, tol_var)


def test_cli_breakpoints_and_consensus_files(tmp_path):
    x = ol.trace(T, K, 1)
    r = run_cli(str(tmp_path), x, FLAGS + " -consensus 8 0.6", ["BP", "CS"])
    assert r.returncode == 0, r.stderr
    sweeps = checker_sweeps(x)
    C, N = bu.counts(sweeps, T)
    assert N == 15 and C.sum() > 0
    assert open(str(tmp_path / "g-breakpoints.csv")).read() == breakpoints_text(C, N)
    assert_consensus_file(str(tmp_path / "g-consensus.csv"), sweeps, C, N, 8, 0.6)
    assert not os.path.exists(str(tmp_path / "g-levels.csv")) and not os.path.exists(str(tmp_path / "g-marginals.csv"))


def test_cli_consensus_default_parameters_and_long_names(tmp_path):
    """no -consensus: window 16, share 0.5; together with the reference's own B (blocks) and C (compression), which keep
    their meaning"""
    x = ol.trace(T, K, 1)
    r = run_cli(str(tmp_path), x, FLAGS, ["consensus", "breakpoints", "B", "C"])
    assert r.returncode == 0, r.stderr
    sweeps = checker_sweeps(x)
    C, N = bu.counts(sweeps, T)
    assert open(str(tmp_path / "g-breakpoints.csv")).read() == breakpoints_text(C, N)
    assert_consensus_file(str(tmp_path / "g-consensus.csv"), sweeps, C, N, 16, 0.5)
    assert os.path.exists(str(tmp_path / "g-blocks.csv")) and os.path.exists(str(tmp_path / "g-compression.csv"))


def test_cli_breaks_three_chains_on_one_gpu(tmp_path):
    """`-chains 3` on one GPU: the chains' counts are merged into the first before the files are written"""
    x = ol.trace(T, K, 1)
    r = run_cli(str(tmp_path), x, "-chains 3 " + FLAGS, ["BP", "CS"], one_gpu=True)
    assert r.returncode == 0, r.stderr
    sweeps = []
    for k in range(3):
        sweeps += checker_sweeps(x, chain=k)
    C, N = bu.counts(sweeps, T)
    assert N == 45
    assert open(str(tmp_path / "g-breakpoints.csv")).read() == breakpoints_text(C, N)
    assert_consensus_file(str(tmp_path / "g-consensus.csv"), sweeps, C, N, 16, 0.5)


def test_cli_breaks_without_a_recording_token(tmp_path):
    x = ol.trace(T, K, 1)
    r = run_cli(str(tmp_path), x, "-s %d -R %d -i F 10 0" % (K, SEED), ["BP", "CS"])
    assert r.returncode == 0, r.stderr
    assert open(str(tmp_path / "g-breakpoints.csv")).read() == ""
    lines = open(str(tmp_path / "g-consensus.csv")).read().splitlines()
    assert len(lines) == 1 and lines[0].split()[:3] == ["0", str(T), "1"]


def test_cli_breaks_refuses_chains_on_several_gpus(tmp_path):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("one GPU")
    x = ol.trace(T, K, 1)
    for outs in (["BP"], ["CS"]):
        r = run_cli(str(tmp_path), x, "-s %d -R %d -chains 2 -i F 10 1" % (K, SEED), outs)
        assert r.returncode == 1 and "different GPUs are not merged yet" in r.stderr
        assert not os.path.exists(str(tmp_path / "g-breakpoints.csv")) and not os.path.exists(str(tmp_path / "g-consensus.csv"))

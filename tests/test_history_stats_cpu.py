"""hml_history_stats (hammlet_amd/csrc/hml_history_stats.h, a header without HIP) as a stand-alone program,
tests/fixtures/history_stats_main.cpp: built with g++ -Wall -Werror, and a second time with the address and undefined-
behaviour sanitizers (nothing is loaded into Python for this), against the numpy restatement of tests/history_util.py.

1e-10 relative: both sides evaluate the same formulas in double, in another order of the additions.  The longest sums have
h = 500 terms of mixed sign (rounding at most 500 2^-53 = 6e-14 of sum |term|), and rho_t = 1 - (W - acov) / var+ keeps that
absolute error; tau sums at most h / 2 of them, so ESS moves by less than 250 * 6e-14 / tau relative - 2e-11 at tau = 1 in the
worst case, typically 1e-14.  The series and their seed are fixed.

The second half runs the helper of the GPU tests on the CPU checker alone: the rows have something to find, and columns 2 + 3
mean what include/hml.h says - the complete-data log-likelihood, block by block."""
import math
import os
import subprocess

import numpy as np
import pytest

from tests import bands_cases as bc
from tests import history_util as hu
from tests import oracle_lib as ol

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "fixtures", "history_stats_main.cpp")
RTOL = 1e-10


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    """the plain build and the sanitizer build of the stand-alone program"""
    d = tmp_path_factory.mktemp("history_stats")
    out = {}
    for name, extra in (("plain", ["-O2"]), ("sanitized", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(d / name)
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + extra + ["-o", exe, SRC], check=True)
        out[name] = exe
    return out


def run(exe, x):
    x = np.atleast_2d(np.asarray(x, np.float64))
    text = "%d %d\n" % x.shape + "\n".join(" ".join(repr(float(v)) for v in row) for row in x) + "\n"
    r = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert r.stderr == "", r.stderr                     # (the sanitizers report there)
    lines = r.stdout.splitlines()
    if r.returncode != 0:
        assert r.returncode == 2 and lines[0].startswith("error "), (r.returncode, r.stdout)
        return dict(error=lines[0][6:])
    head = lines[0].split()
    assert head[0] == "ok" and len(lines) == 1 + x.shape[0]
    per = np.array([[float(v) for v in l.split()] for l in lines[1:]])
    return dict(rhat=float(head[1]), ess=float(head[2]), n_nonfinite=int(head[3]), chain_mean=per[:, 0], chain_sd=per[:, 1])


def close(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.allclose(a[~np.isnan(a)], b[~np.isnan(b)], rtol=RTOL, atol=0)


def check(programs, x, what):
    want = hu.stats(x)
    for name, exe in programs.items():
        got = run(exe, x)
        assert "error" not in got, (what, name, got)
        print("%s (%s): rhat %.12g ess %.12g, restated %.12g %.12g" % (what, name, got["rhat"], got["ess"], want["rhat"], want["ess"]))
        assert got["n_nonfinite"] == want["n_nonfinite"], (what, name)
        for k in ("rhat", "ess", "chain_mean", "chain_sd"):
            assert close(got[k], want[k]), (what, name, k, got[k], want[k])
    return want


@pytest.mark.parametrize("phi", [0.0, 0.5, 0.95])
@pytest.mark.parametrize("shape", [(4, 1000), (1, 64)])
def test_ar1_series(programs, phi, shape):
    want = check(programs, hu.ar1(phi, shape[0], shape[1], seed=1234), "phi %.2f %s" % (phi, shape))
    assert math.isfinite(want["rhat"]) and math.isfinite(want["ess"])
    if shape == (4, 1000):
        # the ESS of an AR(1) series is n (1 - phi) / (1 + phi): the estimate lies within a factor of two of it
        ideal = 4000 * (1 - phi) / (1 + phi)
        assert 0.5 * ideal < want["ess"] < 2.0 * ideal and want["rhat"] < 1.1, (want["ess"], ideal, want["rhat"])


def test_a_shifted_chain_shows(programs):
    want = check(programs, hu.ar1(0.5, 4, 1000, seed=1234, shift=(2, 5.0)), "shifted")
    assert want["rhat"] > 1.5


def test_odd_length_drops_the_middle(programs):
    x = hu.ar1(0.5, 3, 501, seed=7)
    want = check(programs, x, "odd")
    moved = x.copy()
    moved[:, 250] += 100.0                              # the middle value: in neither half
    again = hu.stats(moved)
    assert again["rhat"] == want["rhat"] and again["ess"] == want["ess"]
    for exe in programs.values():
        got = run(exe, moved)
        assert close(got["rhat"], want["rhat"]) and close(got["ess"], want["ess"])


def test_constant_series(programs):
    want = check(programs, np.full((2, 40), 3.25), "constant")
    assert math.isnan(want["rhat"]) and math.isnan(want["ess"]) and np.all(want["chain_sd"] == 0)


def test_one_inf(programs):
    x = hu.ar1(0.5, 2, 100, seed=3)
    x[1, 17] = np.inf
    want = check(programs, x, "one inf")
    assert want["n_nonfinite"] == 1 and math.isnan(want["rhat"]) and math.isnan(want["ess"]) and np.all(np.isfinite(want["chain_mean"]))
    x[0, 3] = np.nan
    x[0, 4] = -np.inf
    assert check(programs, x, "three")["n_nonfinite"] == 3


@pytest.mark.parametrize("n", [6, 7])
def test_too_short(programs, n):
    """h = 3: an error with a message"""
    x = hu.ar1(0.0, 2, n, seed=1)
    with pytest.raises(ValueError):
        hu.stats(x)
    for exe in programs.values():
        got = run(exe, x)
        assert "error" in got and "at least 8 values" in got["error"], got
    assert "error" not in run(programs["plain"], hu.ar1(0.0, 2, 8, seed=1))


# ---- the helper of the GPU tests, on the checker alone ----
SMALL = dict(bc.CASES["k4_mixed"])      # M, S, P, D and F tokens on 20 000 positions


def test_rows_have_something_to_find():
    rows, bounds, _, _, _ = hu.expected("k4_mixed", SMALL)
    n = sum(t[1] for t in SMALL["scheme"] if not isinstance(t, str))
    assert rows.shape == (n, 11) and np.array_equal(rows[:, 0], np.arange(1, n + 1))
    assert set(rows[:, 1]) == {0.0, 1.0}                                    # both methods
    assert np.all(np.isfinite(rows[:, 2:5])) and np.all(rows[:, 6] >= 1) and np.all(rows[:, 7] >= rows[:, 6])
    assert len(set(rows[:, 7])) > 1 and len(set(rows[:, 9])) > 1            # blocks and threshold move
    assert np.all(bounds[:, list(hu.BOUNDED)][np.isfinite(rows[:, list(hu.BOUNDED)])] > 0)
    assert bounds[:, list(hu.BOUNDED)].max() < 1e-6 < np.abs(np.diff(rows[:, 2])).min()   # the bound is far below what moves from sweep to sweep


def test_loglik_means_the_complete_data_likelihood():
    """columns 2 + 3 of every FB sweep = the same likelihood from the checker's blocks, block statistics and states, block by
    block, within 2^-22 sum |addend|: the float rounding of the per-state sums, which the row inherits from the chain on purpose;
    and the transition counts the row is made of are those of the blocks - the self-transitions inside a block included, and the
    transition from state 0 into the first block that the count pass, like the reference, begins with"""
    c = dict(bc.CASES["k5"], T=50000, trace=lambda: ol.trace(50000, 5, 7), scheme=[("F", 12, 1)])
    o, prior = hu.checker(c)
    worst = [0.0]

    def visit(o, method, sweep, row):
        starts, q = o.blocks().astype(np.int64), o.states().astype(np.int64)
        sx, sxx = o.block_stats()
        theta = o.theta()
        A, pi = o.transitions()
        value, scale = hu.loglik_from_blocks(starts, sx, sxx, q, theta[0::2], theta[1::2], A, pi)
        assert abs((row[2] + row[3]) - value) <= 2.0 ** -22 * scale, (sweep, row[2] + row[3], value, scale)
        worst[0] = max(worst[0], abs((row[2] + row[3]) - value) / scale)
        N = np.zeros((c["K"], c["K"]), np.int64)
        np.add.at(N, (q[:-1], q[1:]), 1)
        np.add.at(N, (q, q), np.diff(starts) - 1)
        N[0, q[0]] += 1                                 # (the count pass starts from state 0, like the reference)
        assert np.array_equal(N, o.counts()[0].astype(np.int64)), sweep
        assert row[6] == 1 + np.count_nonzero(q[1:] != q[:-1]) + (1 if q[0] != 0 else 0)
    try:
        rows, _ = hu.walk(o, prior, c["scheme"], visit=visit)
    finally:
        o.close()
    print("largest |row - block by block| / sum |addend| = %.3e (allowed %.3e)" % (worst[0], 2.0 ** -22))
    assert len(rows) == 12


# ---- chains.gathered_history: one process per GPU, here two processes over gloo with stand-ins for the chains ----
class _Rows:
    """what gathered_history needs of a chain: its rows and its device"""
    device = 0

    def __init__(self, rank):
        rng = np.random.RandomState(100 + rank)
        self.rows = rng.standard_normal((5 + 7 * rank, 11))          # unequal lengths
        self.rows[1, 5] = np.inf                                        # ... and bits that a lossy path would not keep
        self.rows[2, 3] = -0.0
        self.rows[:, 10] = rank

    def history(self):
        return self.rows


def _gather_worker(rank, world, port, out):
    import torch.distributed as dist
    from hammlet_amd import chains
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    parts = chains.gathered_history(_Rows(rank))
    np.savez(out % rank, *parts)
    dist.barrier()
    dist.destroy_process_group()


def test_gathered_history_world2(tmp_path):
    import socket
    import torch.multiprocessing as mp
    from hammlet_amd import chains
    assert hu.same_bits(chains.gathered_history(_Rows(1))[0], _Rows(1).rows)      # no process group: the chain's own rows
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    out = str(tmp_path / "rows%d.npz")
    mp.spawn(_gather_worker, args=(2, port, out), nprocs=2, join=True)
    for rank in range(2):                                               # every rank holds every rank's rows, in rank order
        got = np.load(out % rank)
        assert len(got.files) == 2
        for r in range(2):
            assert hu.same_bits(got["arr_%d" % r], _Rows(r).rows), (rank, r)
    x = np.stack([_Rows(r).rows[-5:, 2] for r in range(2)])              # ... cut to the common length: what history_stats takes
    assert x.shape == (2, 5)

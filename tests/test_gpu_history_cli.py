"""`hammlet -O history historysummary [-history-every N] [-history-skip S] -chains 2` (extensions; short forms H, HS):
PREFIXhistorySUFFIX holds a header line and the rows of the chains in order, every double printed with %.17g - parsed back they
are, bit for bit, Chain.history() of the same seed and chain number, which tests/test_gpu_history.py holds against the CPU
checker; PREFIXhistorysummarySUFFIX holds what hammlet_amd.history_summary gives for the same chains."""
import os
import subprocess

import numpy as np
import pytest

from tests.cli_util import CLI, run_cli
from tests import history_util as hu
from tests import oracle_lib as ol

pytestmark = pytest.mark.gpu
T, K, SEED, EVERY = 20000, 3, 4, 2
SCHEME = [("M", 4, 0), ("F", 56, 0)]
FLAGS = "-s %d -R %d -i M 4 0 F 56 0 -chains 2 -history-every %d" % (K, SEED, EVERY)
ROWS = 60 // EVERY


def chains_of(hml, x):
    out = []
    for k in range(2):
        g = hml.Chain(device=0, seed=SEED, chain_id=k)
        g.load(x)
        g.set_model(K, g.autoprior(0.2, 0.9))
        g.set_history(True, EVERY)
        g.sample_prior()
        for m, n, t in SCHEME:
            g.iterate(m, n, t)
        g.sync()
        out.append(g)
    return out


def test_history_files(hml, tmp_path):
    x = ol.trace(T, K, 7)
    r = run_cli(str(tmp_path), x, FLAGS, ["history", "historysummary"])
    assert r.returncode == 0, r.stderr
    chains = chains_of(hml, x)
    lines = open(str(tmp_path / "g-history.csv")).read().splitlines()
    assert lines[0].split("\t") == list(hu.COLS)
    body = [l.split("\t") for l in lines[1:]]
    assert len(body) == 2 * ROWS and all(len(b) == 11 for b in body)
    for j in (0, 1, 6, 7, 8, 10):                                   # whole numbers, printed as such
        assert all(b[j].lstrip("-").isdigit() for b in body), j
    got = np.array([[float(v) for v in b] for b in body])
    want = np.concatenate([g.history() for g in chains])
    assert want.shape == (2 * ROWS, 11) and hu.same_bits(got, want)
    assert np.array_equal(got[:, 10], np.repeat([0.0, 1.0], ROWS)) and np.array_equal(got[:ROWS, 0], np.arange(EVERY, 61, EVERY))
    assert set(got[:, 1]) == {0.0, 1.0}
    # the summary: the second half of the sweeps by default
    summary = [l.split("\t") for l in open(str(tmp_path / "g-historysummary.csv")).read().splitlines()]
    assert [s[0] for s in summary] == [n for n in ("loglik", "logpost", "segments", "blocks") for _ in range(3)]
    for i, name in enumerate(("loglik", "logpost", "segments", "blocks")):
        s = hml.history_summary(chains, name, skip_sweeps=30)
        head, per = summary[3 * i], summary[3 * i + 1: 3 * i + 3]
        assert head[1] == "all" and int(head[4]) == s["n_used"] == ROWS // 2 and int(head[5]) == s["n_nonfinite"] == 0
        for text, value in ((head[2], s["rhat"]), (head[3], s["ess"])):
            assert text == "%.9g" % value, (name, text, value)
        for k in range(2):
            assert per[k][1] == str(k)
            assert hu.same_bits([float(per[k][2]), float(per[k][3])], [s["chain_mean"][k], s["chain_sd"][k]]), (name, k)
    for g in chains:
        g.close()
    # -history-skip
    r = run_cli(str(tmp_path), x, FLAGS + " -history-skip 20", ["HS"])
    assert r.returncode == 0, r.stderr
    assert open(str(tmp_path / "g-historysummary.csv")).read().splitlines()[0].split("\t")[4] == str((60 - 20) // EVERY)
    # a second run refuses to overwrite, each file by its name, before anything runs
    for out, name in (("H", "g-history.csv"), ("HS", "g-historysummary.csv")):
        before = open(str(tmp_path / name)).read()
        r = run_cli(str(tmp_path), x, FLAGS, [out], overwrite=False)
        assert r.returncode == 1 and name in r.stderr and "already exists" in r.stderr, r.stderr
        assert open(str(tmp_path / name)).read() == before


def test_history_flag_errors(tmp_path):
    x = ol.trace(2000, K, 7)
    for flags, message in (("-history-every 0", "-history-every must be a whole number of sweeps, at least 1"),
                           ("-history-every 2.5", "-history-every must be a whole number"),
                           ("-history-skip 1.5", "-history-skip must be a whole number")):
        r = run_cli(str(tmp_path), x, "-s 3 -R 1 -i F 4 0 " + flags, ["H", "HS"])
        assert r.returncode == 1 and message in r.stderr, (flags, r.stderr)
        assert not os.path.exists(str(tmp_path / "g-history.csv"))
    r = subprocess.run([CLI, "-h"], capture_output=True, text=True)
    assert r.returncode == 0 and "-history-every N" in r.stdout and "historysummary" in r.stdout

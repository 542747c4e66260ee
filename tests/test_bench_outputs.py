"""bench.py's plain run and --dump-outputs: the plain line carries the headline alone, --steps sets the timed sweeps, and the
dumped arrays are what the timed chain holds after its last sweep (a chain set up the same way in this process holds the same)."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Chain:
    """what dump_outputs reads of a chain, without a GPU"""

    def __init__(self, B, K=3, seed=0):
        r = np.random.default_rng(seed)
        self.starts = np.concatenate([[0], np.sort(r.choice(np.arange(1, 4 * B), B - 1, replace=False)), [4 * B]]).astype(np.uint32)
        self.st = r.integers(0, K, B).astype(np.int16)
        self.th = r.standard_normal(2 * K).astype(np.float32)
        self.A = r.random((K, K)).astype(np.float32)
        self.pi = r.random(K).astype(np.float32)

    def blocks(self):
        return self.starts

    def states(self):
        return self.st

    def theta(self):
        return self.th

    def transitions(self):
        return self.A, self.pi


def _load(d):
    return {os.path.basename(f)[:-4]: np.load(f) for f in glob.glob(os.path.join(d, "*.npy"))}


def _check_files(d):
    files = glob.glob(os.path.join(d, "*.npy"))
    assert sum(os.path.getsize(f) for f in files) <= bench.DUMP_LIMIT
    for f in files:
        assert np.load(f).dtype in (np.float32, np.float64), f


def test_dump_writes_every_block_when_they_fit(tmp_path):
    c = _Chain(5000)
    bench.dump_outputs(c, str(tmp_path))
    _check_files(str(tmp_path))
    a = _load(str(tmp_path))
    assert "block_index" not in a and a["num_blocks"][0] == 5000
    assert np.array_equal(a["block_starts"], c.starts.astype(np.float64))
    assert np.array_equal(a["block_states"], c.st.astype(np.float32))
    assert np.array_equal(a["theta"], c.th) and np.array_equal(a["transitions"], c.A) and np.array_equal(a["initial"], c.pi)


def test_dump_samples_the_same_blocks_when_they_do_not_fit(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT", 2 << 20)
    c = _Chain(400_000)
    bench.dump_outputs(c, str(tmp_path / "a"))
    bench.dump_outputs(c, str(tmp_path / "b"))
    _check_files(str(tmp_path / "a"))
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)
    idx = a["block_index"].astype(np.int64)
    assert 0 < idx.size < 400_000 and np.all(np.diff(idx) > 0) and a["num_blocks"][0] == 400_000
    assert np.array_equal(a["block_starts"], c.starts[idx].astype(np.float64))
    assert np.array_equal(a["block_states"], c.st[idx].astype(np.float32))


@pytest.mark.gpu
def test_plain_run_and_its_outputs(hml, tmp_path):
    steps, warmup, wl = 9, 4, "c1_1e5_k3"
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
           "--workload", wl, "--dump-outputs", str(tmp_path / "bench")]
    r = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-1500:]
    line = json.loads(lines[0])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in line, key
    assert line["steps"] == steps and line["warmup"] == warmup and line["value"] > 0 and line["ms_per_step"] > 0
    # nothing beyond the headline without --full
    assert "roofline" not in line and "kernels" not in line and line["cpu_baseline"] is None
    _check_files(str(tmp_path / "bench"))
    got = _load(str(tmp_path / "bench"))

    # the headline's chain, step for step
    T, K, levels, sigma, dwell, data_seed = bench.WORKLOADS[wl]
    x = hml.synth_gauss(T, K, levels, sigma, dwell, data_seed, nthreads=4)
    ch = hml.Chain(device=0, seed=1, chain_id=0)
    ch.set_option("weight_keys", 1)
    ch.load(x)
    ch.set_model(K, ch.autoprior(0.2, 0.9))
    ch.sample_prior()
    ch.set_recording(marginals=False)
    ch.iterate("F", warmup, 0)
    ch.sync()
    ch.iterate("F", steps, 0)
    ch.sync()
    bench.dump_outputs(ch, str(tmp_path / "here"))
    ch.close()
    want = _load(str(tmp_path / "here"))
    assert sorted(got) == sorted(want)
    for k in want:
        assert np.array_equal(got[k], want[k]), k

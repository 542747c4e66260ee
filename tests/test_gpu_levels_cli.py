"""`hammlet -O L` (extension): PREFIXlevelsSUFFIX, the denoised trace - per segment its length and, per data dimension, the
posterior mean and standard deviation of the emission level - against the Python API of the same chain."""
import os

import numpy as np
import pytest

from tests.cli_util import run_cli
from tests import oracle_lib as ol

pytestmark = pytest.mark.gpu
T, K, SEED = 100000, 3, 4


def read_levels(path):
    rows = [line.split() for line in open(path).read().splitlines()]
    length = np.array([int(r[0]) for r in rows], np.int64)
    values = np.array([[np.float32(v) for v in r[1:]] for r in rows], np.float32)
    return length, values   # values[:, 2 d] mean, values[:, 2 d + 1] standard deviation


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


def roundtrip(a):
    """float32 -> %.9g -> float32"""
    return np.array([np.float32("%.9g" % v) for v in np.asarray(a, np.float32).ravel()], np.float32).reshape(np.shape(a))


def test_cli_levels_file(hml, tmp_path):
    x = ol.trace(T, K, 1)
    r = run_cli(str(tmp_path), x, "-s %d -R %d -i F 20 0 F 30 2" % (K, SEED), ["M", "L"])
    assert r.returncode == 0, r.stderr
    length, values = read_levels(str(tmp_path / "g-levels.csv"))
    assert length.sum() == T and values.shape == (len(length), 2)
    # both files record the same sweeps: the same segments
    marg = [int(line.split()[0]) for line in open(str(tmp_path / "g-marginals.csv")).read().splitlines()]
    assert list(length) == marg
    g = api_chain(hml, x)
    g.iterate("F", 20, 0)
    g.iterate("F", 30, 2)
    g.sync()
    seg, n, s1, s2 = g.levels_rle()
    assert n == 15 and np.array_equal(seg.astype(np.int64), length)
    mean, sd = hml.levels_mean_sd(n, s1, s2)
    assert np.array_equal(values[:, 0].view(np.uint32), roundtrip(mean[0]).view(np.uint32))
    assert np.array_equal(values[:, 1].view(np.uint32), roundtrip(sd[0]).view(np.uint32))
    assert np.array_equal(roundtrip(mean[0]).view(np.uint32), mean[0].view(np.uint32))   # (%.9g round-trips a float32)


def test_cli_levels_two_chains_on_one_gpu(hml, tmp_path):
    """`-chains 2` on one GPU: the chains' levels are merged into the first before the file is written - the N-weighted
    means of the two chains run separately"""
    x = ol.trace(T, K, 1)
    r = run_cli(str(tmp_path), x, "-s %d -R %d -chains 2 -i F 40 2" % (K, SEED), ["L"], one_gpu=True)
    assert r.returncode == 0, r.stderr
    length, values = read_levels(str(tmp_path / "g-levels.csv"))
    assert length.sum() == T
    a = api_chain(hml, x, chain=0)
    b = api_chain(hml, x, chain=1, attach=a)
    hml.iterate_many([a, b], "F", 40, 2)
    a.sync()
    b.sync()
    segA, nA, a1, a2 = a.levels_rle()
    segB, nB, b1, b2 = b.levels_rle()
    assert nA == nB == 20
    # the file's means are the N-weighted means of the two chains ...
    dense_file = np.repeat(values[:, 0].astype(np.float64), length)
    dense_sep = (np.repeat(a1[0], segA.astype(np.int64)) + np.repeat(b1[0], segB.astype(np.int64))) / (nA + nB)
    scale = max(np.max(np.abs(a1)), np.max(np.abs(b1))) / (nA + nB)
    assert np.max(np.abs(dense_file - dense_sep)) <= 2.0 ** -22 * scale     # (float32 output: half an ulp, with room)
    # ... and exactly what the API's merge gives
    a.merge_levels(b)
    seg, n, s1, s2 = a.levels_rle()
    assert n == 40 and np.array_equal(seg.astype(np.int64), length)
    mean, sd = hml.levels_mean_sd(n, s1, s2)
    assert np.array_equal(values[:, 0].view(np.uint32), mean[0].view(np.uint32))
    assert np.array_equal(values[:, 1].view(np.uint32), sd[0].view(np.uint32))


def test_cli_levels_without_a_recording_token(tmp_path):
    x = ol.trace(T, K, 1)
    r = run_cli(str(tmp_path), x, "-s %d -R %d -i F 10 0" % (K, SEED), ["L"])
    assert r.returncode == 0, r.stderr
    lines = open(str(tmp_path / "g-levels.csv")).read().splitlines()
    assert len(lines) == 1 and lines[0].split()[0] == str(T)
    assert not os.path.exists(str(tmp_path / "g-marginals.csv"))


def test_cli_levels_refuses_chains_on_several_gpus(hml, tmp_path):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("one GPU")
    x = ol.trace(T, K, 1)
    r = run_cli(str(tmp_path), x, "-s %d -R %d -chains 2 -i F 10 1" % (K, SEED), ["L"])
    assert r.returncode == 1 and "different GPUs are not merged yet" in r.stderr
    assert not os.path.exists(str(tmp_path / "g-levels.csv"))

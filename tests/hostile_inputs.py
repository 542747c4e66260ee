"""TEST INFRASTRUCTURE: inputs that are NOT a unit-scale Gaussian trace - scaled, shifted, tied, spiked, tiny and refused ones -
built only from the repository's own generators (ol.trace, ol.synth_depth) and numpy integer arithmetic, so that every machine
regenerates the very floats the reference binary was fed for tests/golden/hostile/ (make_hostile_golden.py keeps their sha256).

INPUTS: name -> (function returning a float32 array, number of states of the model, scheme as run_both of test_gpu_parity.py
takes it).  FAMILY: name -> family; SEED: name -> the chain's seed (`-R`); REFUSED: the names the reference refuses.

Why each family (reference behaviour: src/wavelet.hpp HaarBreakpointWeights, src/Statistics/IntegralArray.hpp, src/HMM.hpp:99-121):
  scale    the prior is not scale-free (`-e` variance 0.2 is absolute): x 2^10 and x 2^40 put every position in a block of its own,
           x 2^-10 and x 2^-40 leave ten blocks of 5000 positions (the rescale factors exp((N-1) log A_ss) reach the denormal range)
  offset   cancellation in (2 mu Sx - Sxx) grows with mean^2 / variance; at 10^4 the reference refuses the input
  depth    integer read depths from 1 to 5000 per position with 3 to 20 states
  ties     integer data: exactly equal Haar coefficients and weights (`!(w < thr)` with w == thr), equal maxima in the maxlet
           transform, equal counts in the arg-max of the segmentation
  spikes   single positions with weights far above the 32-binade window of the 8-bit weight code
  tiny     fewer positions than one group of the summary, one wavefront, one chunk
  refused  the reference's error messages: constant data, zeros, one position, a mean of 10^4 on sigma 0.2
"""
import hashlib
import json
import os
import tarfile

import numpy as np

from tests import oracle_lib as ol


def _base():
    return ol.trace(50000, 3, 1)


def _hash(n, salt):
    """n well-mixed non-negative integers from integer arithmetic alone (the same on every numpy)"""
    i = np.arange(n, dtype=np.uint64) + np.uint64(salt)
    i = (i ^ (i >> np.uint64(15))) * np.uint64(2246822519) % np.uint64(1 << 32)
    i = (i ^ (i >> np.uint64(13))) * np.uint64(3266489917) % np.uint64(1 << 32)
    return (i ^ (i >> np.uint64(16))).astype(np.int64)


def _plateaus(T=60000, noise=False):
    x = (_hash((T + 499) // 500, 7) % 4).repeat(500)[:T]
    if noise:
        x = x + _hash(T, 11) % 3 - 1
    return x.astype(np.float32)


def _spikes():
    x = _base().copy()
    pos = _hash(50, 3) % x.size                       # 0.1 % of the positions
    x[pos] = np.where(np.arange(50) % 2 == 0, 1e3, -1e3).astype(np.float32)
    return x


def _scaled(T, k2=None, f10=None):
    x = ol.trace(T, 3, 1)
    return np.ldexp(x, k2).astype(np.float32) if k2 is not None else (x * np.float32(f10)).astype(np.float32)


F30 = [("F", 30, 1)]
F20 = [("F", 20, 1)]

INPUTS, FAMILY, SEED = {}, {}, {}


def _add(family, name, fn, K, scheme, seed):
    INPUTS[name] = (fn, K, scheme)
    FAMILY[name] = family
    SEED[name] = seed


for _k in (-40, -10, 10, 40):
    _add("scale", "scale_2%s%d" % ("m" if _k < 0 else "p", abs(_k)), (lambda k=_k: _scaled(50000, k2=k)), 3, F30, 9)
_add("scale", "scale_1e3", lambda: _scaled(60000, f10=1e3), 3, F30, 10)
_add("scale", "scale_1em3", lambda: _scaled(60000, f10=1e-3), 3, F30, 10)
for _c in (10, 100, 1000):
    _add("offset", "offset_%d" % _c, (lambda c=_c: (_base() + np.float32(c)).astype(np.float32)), 3, F30, 8)
_add("depth", "depth1_k3", lambda: ol.synth_depth(60000, depth=1.0, seed=3), 3, F20, 4)
_add("depth", "depth15_k5", lambda: ol.synth_depth(60000, depth=15.0, seed=8), 5, [("M", 5, 0), ("F", 20, 2)], 5)
_add("depth", "depth200_k10", lambda: ol.synth_depth(40000, depth=200.0, seed=7), 10, [("F", 12, 2)], 3)
_add("depth", "depth5000_k20", lambda: ol.synth_depth(30000, depth=5000.0, seed=4), 20, [("F", 10, 1)], 1)
_add("depth", "depth15_k20", lambda: ol.synth_depth(60000, depth=15.0, seed=4), 20, F20, 1)
_add("depth", "depth5000_k5", lambda: ol.synth_depth(40000, depth=5000.0, seed=6), 5, [("M", 4, 0), "S", "P", ("F", 12, 1)], 2)
_add("ties", "ties_plateaus", lambda: _plateaus(), 4, F20, 6)
_add("ties", "ties_plateaus_noise", lambda: _plateaus(noise=True), 4, F20, 7)
_add("ties", "ties_alternation", lambda: (np.arange(50000) % 2).astype(np.float32), 2, F20, 3)
_add("ties", "ties_arange", lambda: np.arange(50000, dtype=np.float32), 4, F20, 3)
_add("ties", "ties_rounded", lambda: np.round(_base(), 1).astype(np.float32), 3, F20, 3)
_add("spikes", "spikes", _spikes, 3, F20, 3)
for _T in (2, 3, 5, 7, 15, 16, 17, 63, 64, 65):
    _add("tiny", "tiny_%d" % _T, (lambda T=_T: ol.trace(1000, 3, 2)[:T].copy()), 2, [("F", 10, 1)], 12)
_add("refused", "refused_constant", lambda: np.full(20000, 7.0, np.float32), 3, F20, 3)
_add("refused", "refused_zeros", lambda: np.zeros(20000, np.float32), 3, F20, 3)
_add("refused", "refused_T1", lambda: ol.trace(1000, 3, 2)[:1].copy(), 2, [("F", 10, 1)], 12)
_add("refused", "refused_offset_1e4", lambda: (ol.trace(100000, 3, 1) + np.float32(1e4)).astype(np.float32), 3, F30, 8)

REFUSED = sorted(n for n in INPUTS if FAMILY[n] == "refused")
RUNNABLE = sorted(n for n in INPUTS if FAMILY[n] != "refused")


def family(*names):
    return [n for n in RUNNABLE if FAMILY[n] in names]


def data(name):
    return np.ascontiguousarray(INPUTS[name][0](), np.float32)


def sha256(x):
    return hashlib.sha256(np.ascontiguousarray(x, np.float32).tobytes()).hexdigest()


def flags(name):
    """the reference's command-line flags of the case: `-s K -R seed -i <scheme>`"""
    _, K, scheme = INPUTS[name]
    toks = []
    for t in scheme:
        toks += [t] if isinstance(t, str) else [t[0], str(t[1]), str(t[2])]
    return "-s %d -R %d -i %s" % (K, SEED[name], " ".join(toks))


SMALL_OUTPUTS = ["marginals", "parameters", "compression", "blocks", "sequences"]
LARGE_OUTPUTS = ["marginals", "parameters", "compression"]
# the golden runs of 10^6 positions (read depths, dynamic and static block structure): name -> (synth_depth seed, flags)
MILLION = {
    "depth_1e6_dynamic": (5, "-s 5 -R 1 -i M 20 0 F 30 3"),
    "depth_1e6_static": (6, "-s 5 -R 2 -i M 20 0 S P F 30 3"),
}


def case_input(name):
    """(float32 input, flags, output files) of a golden case of tests/golden/hostile/"""
    if name in MILLION:
        seed, fl = MILLION[name]
        return ol.synth_depth(1_000_000, seed=seed), fl, LARGE_OUTPUTS
    return data(name), flags(name), SMALL_OUTPUTS


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hostile")


def manifest():
    with open(os.path.join(GOLDEN, "manifest.json")) as f:
        return json.load(f)


ARCHIVE = os.path.join(GOLDEN, "outputs.tar.xz")
_archive = None


def archive():
    """member name -> bytes of tests/golden/hostile/outputs.tar.xz (read once)"""
    global _archive
    if _archive is None:
        with tarfile.open(ARCHIVE, "r:xz") as tar:
            _archive = {m.name: tar.extractfile(m).read() for m in tar.getmembers()}
    return dict(_archive)


def assert_golden(entry, case, output, got):
    """`got` holds the bytes the reference binary wrote: size and sha256 from the manifest - and, where the archive keeps the
    reference's file (all but a few large ones), the file itself"""
    e = entry["files"][output]
    if e["stored"]:
        want = archive()["%s/%s.csv" % (case, output)]
        assert hashlib.sha256(want).hexdigest() == e["sha256"], "golden file damaged: %s/%s" % (case, output)
        assert got == want, (case, output)
    assert len(got) == e["bytes"] and hashlib.sha256(got).hexdigest() == e["sha256"], (case, output)


def golden_input(entry, case):
    """the case's input from this module's generators; must be the one the reference binary was fed"""
    x, fl, outs = case_input(case)
    assert sha256(x) == entry["input_sha256"] and fl == entry["flags"], "the generators no longer yield the golden run's input: " + case
    return x


FUZZ_T = [1, 2, 3, 5, 7, 11, 15, 16, 17, 63, 64, 65, 1000, 4097, 30000, 65537]


def fuzz_draw(rng, T=None, T_max=65537):
    """a random member of the families above for the randomised differential run (tests/fuzz_util.py, data="hostile"):
    (description, float32 array of T positions); T from FUZZ_T (1 ... 16 included) unless given"""
    if T is None:
        T = int(rng.choice([t for t in FUZZ_T if t <= T_max]))
    kind = str(rng.choice(["scale2", "scale10", "offset", "depth", "plateaus", "plateaus_noise", "alternation", "arange", "rounded", "spikes"]))
    seed = int(rng.integers(1, 1000))
    if kind == "scale2":
        k = int(rng.choice([-40, -10, 10, 40]))
        return "%s^%d" % (kind, k), np.ldexp(ol.trace(T, 3, seed), k).astype(np.float32)
    if kind == "scale10":
        f = float(rng.choice([1e3, 1e-3]))
        return "%s*%g" % (kind, f), (ol.trace(T, 3, seed) * np.float32(f)).astype(np.float32)
    if kind == "offset":
        c = float(rng.choice([10, 100, 1000]))
        return "%s+%g" % (kind, c), (ol.trace(T, 3, seed) + np.float32(c)).astype(np.float32)
    if kind == "depth":
        d = float(rng.choice([1, 15, 200, 5000]))
        return "%s=%g" % (kind, d), ol.synth_depth(T, depth=d, seed=seed)
    if kind == "plateaus":
        return kind, _plateaus(T)
    if kind == "plateaus_noise":
        return kind, _plateaus(T, noise=True)
    if kind == "alternation":
        return kind, (np.arange(T) % 2).astype(np.float32)
    if kind == "arange":
        return kind, np.arange(T, dtype=np.float32)
    if kind == "rounded":
        return kind, np.round(ol.trace(T, 3, seed), 1).astype(np.float32)
    x = ol.trace(T, 3, seed).copy()
    n = max(1, T // 1000)
    x[_hash(n, seed) % T] = np.where(np.arange(n) % 2 == 0, 1e3, -1e3).astype(np.float32)
    return kind, x

"""The HIP path against the CPU checker on inputs that are NOT a unit-scale Gaussian trace (tests/hostile_inputs.py): scaled by
2^+-10, 2^+-40 and 10^+-3, shifted by 10 / 100 / 1000, read depths of 1 to 5000 with 3 to 20 states, integer data full of ties,
spikes of +-10^3, 2 to 65 positions, and the inputs the reference refuses.  The checker is pinned on files the unmodified
reference binary wrote for the very same inputs (tests/test_hostile_golden_cpu.py), so a difference here is the product's.

Mechanisms whose correctness depends on the magnitude and the tie structure of the input, and the case that holds each:
  hml_weight_key's clamps at 0 / 255 and the fall-back to the float stream   spikes, scale_2p40 / scale_2m40, weight_keys = 2
  `!(w[t] < thr)` with w == thr, equal maxima in the maxlet transform            ties_* (integer data)
  cancellation in (2 mu Sx - Sxx), Kahan cells of the integral array             offset_100 / offset_1000, depth5000_*
  rescale factors exp((N-1) log A_ss) in the denormal range, all-zero rows      scale_2m10 / scale_2m40, ties_alternation
  every position a block without a forced threshold (weakly compressed path)    scale_2p10 / scale_2p40 / scale_1e3, depth200 / depth5000
  fewer positions than a group of the summary, a wavefront, a chunk             tiny_*
  arg-max with equal counts (first maximum, strict >)                            ties_* through max_segmentation
"""
import os
import subprocess
import tempfile

import numpy as np
import pytest

from tests import hostile_inputs as hi
from tests import oracle_lib as ol
from tests.test_gpu_parity import bits, make_pair, run_both, setup_model

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(REPO, "hammlet_amd", "hammlet")
MANIFEST = hi.manifest()
_CHECKER = {}      # what the checker left, by case: it runs once however many GPU variants are compared with it


def snapshot(c, hml=None, probes=True):
    """everything the comparison looks at, as bytes-comparable values; hml: the product's chain, else the checker's.
    (The threshold is compared by next_threshold: the product derives it from the new parameters at the end of a sweep,
    the checker at the start of the next one.)"""
    s, q = c.block_stats()
    A, pi = c.transitions()
    out = {"blocks": np.asarray(c.blocks()), "sum": bits(s), "sumsq": bits(q), "states": np.asarray(c.states()), "theta": bits(c.theta()),
           "A": bits(A), "pi": bits(pi)}
    if probes:
        out["emission"] = bits(c.block_loglik() if hml else c.loglik())
        out["forward"] = bits(c.forward_rows())
    out["marginals"] = hml.marginals_text(*c.marginals_rle()) if hml else c.text("marginals")
    return out


def next_threshold(o):
    """the threshold of the checker's NEXT sweep - what the product holds once a sweep is over; ends the checker's chain"""
    o.iterate("F", 1, 0)
    return bits(np.float32(o.threshold()))


def same(a, b, what):
    assert sorted(a) == sorted(b)
    for k in a:
        if isinstance(a[k], str):
            assert a[k] == b[k], (what, k)
        else:
            assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), (what, k)


def run_pair(hml, x, K, seed, scheme, weight_keys=None, key=None, probes=True):
    """first sweep with probes on (emission terms, forward rows), then the scheme: (checker, product) snapshots after each"""
    want = _CHECKER.get(key) if key is not None else None
    xx, o, g = make_pair(hml, x.size, K, 0, seed, x=x, weight_keys=weight_keys)
    if want is not None:
        o.close()
        o = None
        g.set_model(K, g.autoprior(0.2, 0.9))
    else:
        setup_model(o, g, K)
    g._pending_prior = True
    if o is not None:
        o.set_record(marginals=True)
        o.set_probes(probes)
    g.enable_probes(probes)
    got = []
    for part in ([("F", 1, 0)], scheme):
        if o is not None:
            run_both(o, g, part)
        else:
            run_both(_Silent(), g, part)
        got.append(snapshot(g, hml, probes))
        if o is not None:
            want = (want or []) + [snapshot(o, probes=probes)]
    got[1]["threshold"] = bits(np.float32(g.threshold()))
    if o is not None:
        want[1]["threshold"] = next_threshold(o)
        o.close()
    if key is not None:
        _CHECKER[key] = want
    g.close()
    return want, got


class _Silent:
    """stands where the checker stood once its results are kept"""
    def token(self, t):
        pass

    def iterate(self, m, n, t):
        pass


@pytest.mark.parametrize("keys", [1, 2, 0])
@pytest.mark.parametrize("name", hi.RUNNABLE)
def test_default_path_bit_for_bit(hml, name, keys):
    """Blocks, block statistics, states, theta / A / pi bits, threshold, marginals text, emission terms and forward rows (after the
    first sweep and after the scheme) equal the device-mode checker's, with the weight summary on (1), forced - never the float
    stream, so the key clamps decide (2) - and off (0)."""
    fn, K, scheme = hi.INPUTS[name]
    want, got = run_pair(hml, hi.data(name), K, hi.SEED[name], scheme, weight_keys=keys, key=("default", name))
    same(want[0], got[0], (name, keys, "first sweep"))
    same(want[1], got[1], (name, keys, "scheme"))


@pytest.mark.parametrize("dense_L", [16, 8])
@pytest.mark.parametrize("name", hi.RUNNABLE)
def test_weakly_compressed_geometry_on_every_family(hml, monkeypatch, name, dense_L):
    """The forward geometry of sweeps with many blocks (HML_DENSE_MIN_BLOCKS lowered to 1, chunks of 16 and 8) on every input:
    the results are the checker's, which are those of the default geometry."""
    monkeypatch.setenv("HML_DENSE_MIN_BLOCKS", "1")
    monkeypatch.setenv("HML_FWD_CHUNK_DENSE", str(dense_L))
    fn, K, scheme = hi.INPUTS[name]
    want, got = run_pair(hml, hi.data(name), K, hi.SEED[name], scheme, key=("default", name))
    same(want[0], got[0], (name, dense_L, "first sweep"))
    same(want[1], got[1], (name, dense_L, "scheme"))


def test_weakly_compressed_path_at_its_natural_threshold(hml):
    """5 10^6 positions scaled by 2^10: the first sweep finds (nearly) every position a block, above the 2^22 blocks from which the
    sweep takes the weakly compressed path by itself - no threshold forced, no weight multiplier - and the following sweeps, whose
    states have taken up the data's variance, fall back below it."""
    T, K = 5_000_000, 3
    x = np.ldexp(ol.trace(T, 3, 1), 10).astype(np.float32)
    want, got = run_pair(hml, x, K, 9, [("F", 3, 1)], probes=False)
    assert got[0]["blocks"].size - 1 > (1 << 22) > got[1]["blocks"].size - 1
    same(want[0], got[0], "first sweep")
    same(want[1], got[1], "scheme")


WIDE_SCHEME = [("F", 3, 1), "S", ("F", 2, 1), "D", ("F", 2, 1)]
WIDE_T = 16000     # the first positions of every input: 40 states on every position a block cost the checker seconds per 10^4


@pytest.mark.parametrize("K,force", [(20, False), (40, False), (5, True)])
@pytest.mark.parametrize("name", hi.family("scale", "depth", "ties", "tiny", "spikes"))
def test_path_for_many_states(hml, monkeypatch, name, K, force):
    """hml_k_wide.h / hml_k_wide_lanes.h (20 and 40 states; 5 states sent there by HML_WIDE=1) on scale, depth, ties and tiny
    (the first 16000 positions of each) - and on spikes, where rows of the backward draw are all zero (the checker's chain changes
    when its hml_categorical answers K - 1 instead of 0 there, so the kernels' own forms of that rule are held by it)."""
    if force:
        monkeypatch.setenv("HML_WIDE", "1")
    want, got = run_pair(hml, hi.data(name)[:WIDE_T].copy(), K, hi.SEED[name], WIDE_SCHEME, key=("wide", name, K))
    same(want[0], got[0], (name, K, "first sweep"))
    same(want[1], got[1], (name, K, "scheme"))


@pytest.mark.parametrize("attached", [True, False])
@pytest.mark.parametrize("name", hi.family("depth", "ties", "spikes") + ["scale_2p10"])
def test_many_chains_are_the_chains_run_alone(hml, name, attached):
    """hml_iterate_many, four chains over one construction (hml_attach_observations) and with private ones: every chain stays the
    chain the checker runs alone - blocks, block statistics, states, parameters, threshold, marginals."""
    x = hi.data(name)
    K = min(hi.INPUTS[name][1], 5)
    seed, n = hi.SEED[name], 4
    key = ("many", name)
    want = _CHECKER.get(key)
    pairs = []
    for chain in range(n):
        g = hml.Chain(device=0, seed=seed, chain_id=chain)
        if attached and chain > 0:
            g.attach(pairs[0][1])
        else:
            g.load(x)
        o = None
        if want is None:
            o = ol.OracleChain(K=K, seed=seed, chain=chain, rng=ol.RNG_CTR, math=ol.MATH_DEV, reduce=ol.REDUCE_DEV)
            o.load(x)
            setup_model(o, g, K)
            o.token("F")
            o.set_record(marginals=True)
        else:
            g.set_model(K, g.autoprior(0.2, 0.9))
        g.sample_prior()
        pairs.append((o, g))
    gs = [g for _, g in pairs]
    for method, iters, thin in (("F", 8, 2), ("P", 0, 0), ("F", 4, 1)):
        if method == "P":
            for o, g in pairs:
                if o is not None:
                    o.token("P")
                    o.token("F")
                g.sample_prior()
            continue
        for o, _ in pairs:
            if o is not None:
                o.iterate(method, iters, thin)
        hml.iterate_many(gs, method, iters, thin)
    for g in gs:
        g.sync()
    if want is None:
        want = _CHECKER[key] = [snapshot(o, probes=False) for o, _ in pairs]
        for w, (o, _) in zip(want, pairs):
            w["threshold"] = next_threshold(o)
            o.close()
    for chain, g in enumerate(gs):
        got = snapshot(g, hml, probes=False)
        got["threshold"] = bits(np.float32(g.threshold()))
        same(want[chain], got, (name, attached, chain))
    for g in reversed(gs):
        g.close()


@pytest.mark.parametrize("case", sorted(c for c in MANIFEST if MANIFEST[c]["status"] == 0))
def test_cli_compat_writes_the_reference_binarys_files_on_hostile_inputs(case):
    """`hammlet -compat -raw` with the flags of a golden run of tests/golden/hostile/ against the bytes the unmodified reference
    binary wrote: from the GPU, mt19937 and libm and all."""
    m = MANIFEST[case]
    x = hi.golden_input(m, case)
    with tempfile.TemporaryDirectory() as tmp:
        raw = os.path.join(tmp, "in.f32")
        x.tofile(raw)
        r = subprocess.run([CLI, "-compat", "-raw", raw, "-o", os.path.join(tmp, "g-"), ".csv", "-a"] + m["flags"].split() + ["-O"] + m["outputs"],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        for o in m["outputs"]:
            with open(os.path.join(tmp, "g-%s.csv" % o), "rb") as f:
                hi.assert_golden(m, case, o, f.read())


@pytest.mark.parametrize("compat", [False, True])
@pytest.mark.parametrize("case", hi.REFUSED)
def test_refused_inputs_through_the_cli_and_the_c_abi(hml, case, compat):
    """constant data, zeros, one position, a mean of 10^4 on sigma 0.2: the command line ends with the reference's message and a
    non-zero status, hml_autoprior fails with the same message."""
    m = MANIFEST[case]
    x = hi.golden_input(m, case)
    message = m["stderr"].split("[ERROR] ")[1].split("\n")[0]
    with tempfile.TemporaryDirectory() as tmp:
        raw = os.path.join(tmp, "in.f32")
        x.tofile(raw)
        r = subprocess.run([CLI] + (["-compat"] if compat else []) + ["-raw", raw, "-o", os.path.join(tmp, "g-"), ".csv", "-a"] + m["flags"].split() +
                           ["-O"] + hi.SMALL_OUTPUTS, capture_output=True, text=True)
    assert r.returncode != 0 and r.returncode == m["status"]
    assert r.stderr == m["stderr"]
    g = hml.Chain(device=0, seed=hi.SEED[case])
    if compat:
        g.set_option("compat", 1)
    g.load(x)
    with pytest.raises(hml.HmlError) as err:
        g.autoprior(0.2, 0.9)
    assert message in str(err.value)
    g.close()


@pytest.mark.parametrize("name", hi.family("ties"))
def test_device_segmentation_on_equal_counts(hml, name):
    """hml_max_segmentation against the restated reference tool on the marginals of integer data, where equal counts are
    common: first maximum, strict `>`."""
    from tests.test_gpu_maxseg import tool_text
    fn, K, scheme = hi.INPUTS[name]
    x = hi.data(name)
    g = hml.Chain(device=0, seed=hi.SEED[name])
    g.load(x)
    g.set_model(K, g.autoprior(0.2, 0.9))
    g.sample_prior()
    g.iterate("F", 12, 1)       # an even number of recorded sweeps: two states can share a position equally
    g.sync()
    seg, cnt = g.marginals_rle()
    run_len, run_state = g.max_segmentation()
    assert int(run_len.sum()) == x.size
    assert tool_text(run_len, run_state) == ol.max_segmentation_text(hml.marginals_text(seg, cnt))
    g.close()

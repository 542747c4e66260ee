"""Breakpoint posteriors and the consensus segmentation on the GPU (hml_k_breaks.h behind hml_set_break_recording /
hml_breaks_list / hml_breaks_dense_device / hml_breaks_merge / hml_breaks_consensus, and hml_levels_on_segments).  The
expected values come from the CPU CHECKER - its blocks, states and theta after every recorded sweep, stepped one sweep per
call - through tests/breaks_util.py; never from the product.  Every comparison is EXACT, integers and float bits alike,
except hml_levels_on_segments, which is held to the bound of breaks_util.segment_bounds (DESIGN.md 3c'': from the
arithmetic, not from a measurement).  tests/test_breaks_cpu.py shows that every consensus case here is non-vacuous."""
import numpy as np
import pytest

from tests import breaks_cases as bc
from tests import breaks_util as bu
from tests import hostile_inputs as hi
from tests import levels_util as lu
from tests import oracle_lib as ol

pytestmark = pytest.mark.gpu


def bits32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def gpu_chain(hml, c, x, chain=0, options=(), breaks=True, levels=False, attach=None):
    g = hml.Chain(device=0, seed=c["seed"], chain_id=chain)
    for name, value in options:
        g.set_option(name, value)
    if c["compat"]:
        g.set_option("compat", 1)
    if attach is not None:
        g.attach(attach)
    else:
        if c["D"] > 1:
            g.set_dimensions(c["D"], c["P"])
        g.load(x)
    g.set_model(c["K"], g.autoprior(0.2, 0.9))
    if breaks:
        g.set_break_recording(True)
    if levels:
        g.set_level_recording(True)
    g._pending_prior = True
    return g


def gpu_token(g, tok):
    """one scheme token on the GPU chain: ONE iterate call per sweep token"""
    if g._pending_prior:
        g.sample_prior()
        g._pending_prior = False
    if tok == "P":
        g._pending_prior = True
    elif tok == "S":
        g.set_static_blocks()
    elif tok == "D":
        g.set_dynamic(True)
    else:
        g.iterate(*tok)


def run_gpu(g, scheme):
    for tok in scheme:
        gpu_token(g, tok)
    g.sync()


def assert_same_chain(o, g, what):
    assert np.array_equal(o.blocks(), g.blocks()) and np.array_equal(o.states(), g.states()), what
    assert np.array_equal(o.theta().view(np.uint32), g.theta().view(np.uint32)), what


def assert_list(g, C, N, what=""):
    pos, cnt, n = g.breaks_list()
    want_pos, want_cnt = bu.listing(C)
    assert n == N, (what, n, N)
    assert pos.dtype == np.uint32 and cnt.dtype == np.uint32
    assert np.array_equal(pos.astype(np.int64), want_pos), what
    assert np.array_equal(cnt.astype(np.int64), want_cnt), what
    return pos, cnt


def assert_dense(g, C, N, windows, what=""):
    import torch
    T = len(C)
    for w in windows:
        out = torch.full((T,), -7.0, dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()      # (the fill runs on torch's stream, the read-out on the chain's)
        g.breaks_dense(out.data_ptr(), w)
        got = out.cpu().numpy()
        assert np.array_equal(bits32(got), bits32(bu.dense(C, N, w))), (what, w)


def assert_consensus(g, C, N, pairs, what=""):
    for w, P in pairs:
        need = bu.min_count_of(P, N)
        pos, mass, peak = g.breaks_consensus(w, need)
        (want_pos, want_mass, want_peak), _ = bu.consensus(C, w, need)
        assert np.array_equal(pos.astype(np.int64), want_pos), (what, w, need)
        assert np.array_equal(mass.astype(np.int64), want_mass), (what, w, need)
        assert np.array_equal(peak.astype(np.int64), want_peak), (what, w, need)


def assert_all(g, sweeps, T, what=""):
    C, N = bu.counts(sweeps, T)
    assert_list(g, C, N, what)
    assert_dense(g, C, N, bc.DENSE_WINDOWS, what)
    assert_consensus(g, C, N, bc.CONSENSUS, what)
    return C, N


def assert_on_segments(g, sweeps, T, D, P, cuts, what=""):
    """hml_levels_on_segments against the dense sums of levels_util, within the bound of the arithmetic; twice, same bits"""
    S1, S2, boundary, N = lu.accumulate(sweeps, T, D=D, P=P)
    M = int(boundary.sum())
    want1, length = bu.segment_sums(S1, cuts)
    want2, _ = bu.segment_sums(S2, cuts)
    s1, s2 = g.levels_on_segments(cuts)
    assert s1.shape == (D, len(cuts) + 1) and s2.shape == s1.shape
    B1, B2 = bu.segment_bounds(M, N, lu.max_abs_mean(sweeps), T, length)
    for d in range(D):
        e1, e2 = np.abs(s1[d] - want1[d]), np.abs(s2[d] - want2[d])
        k1, k2 = int(np.argmax(e1 / B1)), int(np.argmax(e2 / B2))
        print("%s d=%d M=%d N=%d cuts=%d: |S1 error| %.3g (bound %.3g), |S2 error| %.3g (bound %.3g)" %
              (what, d, M, N, len(cuts), e1[k1], B1[k1], e2[k2], B2[k2]))
        assert np.all(e1 <= B1), (what, d, k1, e1[k1], B1[k1])
        assert np.all(e2 <= B2), (what, d, k2, e2[k2], B2[k2])
    again = g.levels_on_segments(cuts)
    assert np.array_equal(bits64(again[0]), bits64(s1)) and np.array_equal(bits64(again[1]), bits64(s2)), what
    return s1, s2


@pytest.mark.parametrize("name", sorted(bc.CASES))
def test_breaks_match_checker(hml, monkeypatch, name):
    """list, dense (windows 0, 1, 16) and consensus (three pairs) of every chain of tests/breaks_cases.py - default path with
    2, 5 and 10 states, the wide path, compat mode, `C 2 2`, the mixed scheme, the weakly compressed geometry - and
    hml_levels_on_segments with the consensus' cuts and with arbitrary ones"""
    c = bc.CASES[name]
    for k, v in c["env"].items():
        monkeypatch.setenv(k, v)
    x = c["trace"]()
    T = c["T"]
    o = bc.checker(name)
    g = gpu_chain(hml, c, x, levels=True)
    sweeps = bc.checker_sweeps(o, c["scheme"])
    run_gpu(g, c["scheme"])
    assert_same_chain(o, g, name)
    C, N = assert_all(g, sweeps, T, name)
    assert len(bu.listing(C)[0]) > 0
    P = c["P"] if c["D"] > 1 else c["K"]
    w, frac = bc.CONSENSUS[1]
    cons = g.breaks_consensus(w, bu.min_count_of(frac, N))[0]
    assert len(cons) > 0
    assert_on_segments(g, sweeps, T, c["D"], P, cons, name + " consensus cuts")
    assert_on_segments(g, sweeps, T, c["D"], P, bc.arbitrary_cuts(T), name + " arbitrary cuts")
    both = np.union1d(cons.astype(np.int64), bc.arbitrary_cuts(T))
    assert_on_segments(g, sweeps, T, c["D"], P, both, name + " both")
    assert_on_segments(g, sweeps, T, c["D"], P, np.zeros(0, np.int64), name + " no cuts")
    g.close()
    o.close()


def test_breaks_iterate_many_and_merge(hml):
    """three chains attached to one trace through hml_iterate_many: each chain's breaks are the checker's chain run alone;
    breaks_merge of the three = the sum of the three lists, and the destination records on"""
    name = "k5"
    c = dict(bc.CASES[name])
    T = c["T"]
    x = c["trace"]()
    scheme = [("F", 12, 0), ("F", 18, 3)]
    first = gpu_chain(hml, c, x, chain=0)
    chains = [first] + [gpu_chain(hml, c, x, chain=k, attach=first) for k in (1, 2)]
    for g in chains:
        g.sample_prior()
        g._pending_prior = False
    for m, n, t in scheme:
        hml.iterate_many(chains, m, n, t)
    total = np.zeros(T, np.int64)
    for k, g in enumerate(chains):
        g.sync()
        o = bc.checker(name, chain=k)
        sweeps = bc.checker_sweeps(o, scheme)
        assert_same_chain(o, g, k)
        C, N = assert_all(g, sweeps, T, "iterate_many chain %d" % k)
        assert N == 6
        total += C
        o.close()
    before = chains[1].breaks_list()
    chains[0].breaks_merge(chains[1])
    chains[0].breaks_merge(chains[2])
    assert_list(chains[0], total, 18, "merged")
    assert_dense(chains[0], total, 18, bc.DENSE_WINDOWS, "merged")
    assert_consensus(chains[0], total, 18, bc.CONSENSUS, "merged")
    after = chains[1].breaks_list()
    assert after[2] == before[2] and np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1])   # the source is unchanged
    chains[0].iterate("F", 2, 1)
    chains[0].sync()
    assert chains[0].breaks_list()[2] == 20
    for g in chains[::-1]:
        g.close()


def test_breaks_survive_buffer_growth(hml):
    """per-block buffers sized for 64 blocks: the chain halts, grows and runs the sweeps again (hml_settle) - every recorded
    sweep is counted once"""
    c = dict(bc.CASES["k2"])
    c["scheme"] = [("M", 4, 1), ("F", 16, 2)]
    T = c["T"]
    x = c["trace"]()
    o = bc.checker(c)
    sweeps = bc.checker_sweeps(o, c["scheme"])
    g = gpu_chain(hml, c, x, options=(("max_blocks", 64),))
    run_gpu(g, c["scheme"])
    assert g.stats()["buffer_growths"] > 0
    assert_same_chain(o, g, "growth")
    C, N = assert_all(g, sweeps, T, "growth")
    assert N == 12
    g.close()
    o.close()


HOSTILE = hi.family("ties", "spikes", "tiny")


@pytest.mark.parametrize("name", HOSTILE)
def test_breaks_on_hostile_inputs(hml, name):
    """integer data with exact ties, spikes, traces of 2 to 65 positions (T = 2: the only possible breakpoint is t = 1; a chain
    that recorded but saw none returns an empty list, not an error).  These inputs are outside the non-vacuity table of
    tests/test_breaks_cpu.py: whatever the checker's chain gives - also nothing at all - is what the GPU must return."""
    fn, K, scheme = hi.INPUTS[name]
    x = hi.data(name)
    T = x.size
    c = dict(T=T, K=K, seed=hi.SEED[name], scheme=scheme, trace=x, D=1, P=None, compat=False, env={})
    o = bc.checker(c)
    sweeps = bc.checker_sweeps(o, scheme)
    g = gpu_chain(hml, c, x)
    run_gpu(g, scheme)
    assert_same_chain(o, g, name)
    C, N = assert_all(g, sweeps, T, name)
    pos, cnt, n = g.breaks_list()
    print("%s: T=%d N=%d breaks at %d positions" % (name, T, N, len(pos)))
    if T == 2:
        assert set(pos.tolist()) <= {1}
    g.close()
    o.close()


def test_breaks_toggled_in_mid_scheme(hml):
    """off for the second token, on again for the third: what was accumulated stays, what ran in between is not counted"""
    c = dict(bc.CASES["k2"])
    scheme = [("F", 8, 2), ("F", 6, 1), ("M", 4, 1), ("F", 9, 3)]
    on = [True, False, True, True]
    T = c["T"]
    x = c["trace"]()
    o = bc.checker(c)
    sweeps = bc.checker_sweeps(o, scheme, recording=on)
    g = gpu_chain(hml, c, x, breaks=False)
    g.profile_enable(2)
    for tok, flag in zip(scheme, on):
        g.set_break_recording(flag)
        gpu_token(g, tok)
    g.sync()
    assert_same_chain(o, g, "toggled")
    C, N = assert_all(g, sweeps, T, "toggled")
    assert N == 4 + 4 + 3 and g.recorded_sweeps() == 4 + 6 + 4 + 3
    assert g.profile_get("breaks")[1] == N
    g.close()
    o.close()


def test_breaks_off_is_invisible(hml):
    """a chain with the recording off is bit-identical in blocks, states and theta to one with it on and launches no break
    kernel; its read-outs are refused"""
    c = bc.CASES["k4_mixed"]
    x = c["trace"]()
    chains = []
    for flag in (False, True):
        g = gpu_chain(hml, c, x, breaks=flag)
        g.profile_enable(2)
        run_gpu(g, c["scheme"])
        chains.append(g)
    off, on = chains
    assert np.array_equal(off.blocks(), on.blocks()) and np.array_equal(off.states(), on.states())
    assert np.array_equal(off.theta().view(np.uint32), on.theta().view(np.uint32))
    seg0, cnt0 = off.marginals_rle()
    seg1, cnt1 = on.marginals_rle()
    assert np.array_equal(seg0, seg1) and np.array_equal(cnt0, cnt1)
    n_rec = on.recorded_sweeps()
    assert n_rec == off.recorded_sweeps() == 10
    assert off.profile_get("breaks")[1] == 0 and on.profile_get("breaks")[1] == n_rec
    assert off.profile_get("marginals")[1] == on.profile_get("marginals")[1] > 0
    assert off.profile_get("levels")[1] == 0 and on.profile_get("levels")[1] == 0
    for call in (off.breaks_list, lambda: off.breaks_consensus(4, 1)):
        with pytest.raises(hml.HmlError) as e:
            call()
        assert e.value.code == 1 and "hml_set_break_recording" in str(e.value)
    for g in chains:
        g.close()


def test_breaks_error_paths(hml):
    import torch
    c = bc.CASES["k4_mixed"]
    T = c["T"]
    x = c["trace"]()
    g = gpu_chain(hml, c, x, breaks=True, levels=False)
    run_gpu(g, [("F", 6, 2)])
    # levels were never recorded by this context
    with pytest.raises(hml.HmlError) as e:
        g.levels_on_segments([10, 20])
    assert e.value.code == 1 and "hml_set_level_recording" in str(e.value)
    # never recorded breaks: list, dense, consensus, and as the source of a merge
    n = gpu_chain(hml, c, x, breaks=False, levels=True)
    run_gpu(n, [("F", 6, 2)])
    out = torch.zeros(T, dtype=torch.float32, device="cuda:0")
    for call in (n.breaks_list, lambda: n.breaks_dense(out.data_ptr(), 0), lambda: n.breaks_consensus(1, 1), lambda: g.breaks_merge(n)):
        with pytest.raises(hml.HmlError) as e:
            call()
        assert e.value.code == 1 and "hml_set_break_recording" in str(e.value)
    # unsorted, repeated and out-of-range cuts
    for cuts in ([20, 10], [10, 10], [0, 10], [10, T], [T + 5]):
        with pytest.raises(hml.HmlError) as e:
            n.levels_on_segments(cuts)
        assert e.value.code == 1, cuts
    assert n.levels_on_segments([1, T - 1])[0].shape == (1, 3)
    # other positions: the merge is refused; a context is not merged into itself
    c2 = dict(c, T=T // 2)
    h = gpu_chain(hml, c2, x[:T // 2])
    run_gpu(h, [("F", 4, 1)])
    for src in (h, g):
        with pytest.raises(hml.HmlError) as e:
            g.breaks_merge(src)
        assert e.value.code == 1
    # asked for, nothing recorded yet: an empty list, N = 0, NaN everywhere, nothing selected
    z = gpu_chain(hml, c, x)
    z.sample_prior()
    z.iterate("F", 3, 0)
    z.sync()
    pos, cnt, nrec = z.breaks_list()
    assert len(pos) == 0 and len(cnt) == 0 and nrec == 0
    z.breaks_dense(out.data_ptr(), 3)
    assert np.all(np.isnan(out.cpu().numpy()))
    assert len(z.breaks_consensus(3, 0)[0]) == 0
    for q in (g, n, h, z):
        q.close()

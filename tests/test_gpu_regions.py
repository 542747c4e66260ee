"""Joint posteriors over caller-given regions on the GPU (hml_k_regions.h behind hml_set_regions / hml_regions_read /
hml_regions_add / hml_regions_merge).  The expected sums come from the CPU CHECKER - its blocks, states and theta after every
recorded sweep, stepped one sweep per call - accumulated by tests/regions_util.py; never from the product.  Integers are
compared exactly, the double sums under the bound of tests/regions_util.py, which is computed from T, B, N, max |mean| and the
region's length alone (the largest error is printed next to it).  tests/test_regions_cpu.py shows on the checker alone that
the cases have something to find."""
import numpy as np
import pytest

from tests import bands_cases as bc
from tests import oracle_lib as ol
from tests import regions_util as ru

pytestmark = pytest.mark.gpu

DOUBLES = ("level_sum", "level_sq")


def gpu_chain(hml, c, chain=0, options=(), attach=None, regions=None, edges="case", trace=None, seed=None):
    g = hml.Chain(device=0, seed=c["seed"] if seed is None else seed, chain_id=chain)
    for name, value in options:
        g.set_option(name, value)
    if c["compat"]:
        g.set_option("compat", 1)
    if attach is not None:
        g.attach(attach)
    else:
        if c["D"] > 1:
            g.set_dimensions(c["D"], c["P"])
        x = trace if trace is not None else c["trace"]
        g.load(x() if callable(x) else x)
    g.set_model(c["K"], g.autoprior(0.2, 0.9))
    if regions is not None:
        g.set_regions(regions[0], regions[1], c["edges"] if isinstance(edges, str) else edges)
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


def gpu_run(g, scheme):
    for tok in scheme:
        gpu_token(g, tok)
    g.sync()
    return g


def shape_of(c):
    return c["D"], (c["P"] if c["D"] > 1 else None)


def same_bits(a, b):
    """two regions() results: N, integers and the bit patterns of the doubles"""
    return a["N"] == b["N"] and all(np.array_equal(a[k], b[k]) for k in ("whole", "breaks_sum", "breaks_sq", "inband")) and \
        all(np.array_equal(a[k].view(np.uint64), b[k].view(np.uint64)) for k in DOUBLES)


def run_case(hml, c, what="", options=(), regions=None, region_seed=0):
    """blocks, states and theta bits equal to the checker's first - which also shows that the recording does not disturb the
    chain - then the regions"""
    D, P = shape_of(c)
    o = bc.checker(c)
    try:
        sweeps = bc.checker_sweeps(o, c["scheme"])
        if regions is None:
            regions = ru.standard_regions(c["T"], sweeps[-1], seed=region_seed)
        g = gpu_run(gpu_chain(hml, c, options=options, regions=regions), c["scheme"])
        assert np.array_equal(o.blocks(), g.blocks()) and np.array_equal(o.states(), g.states()), what
        assert np.array_equal(o.theta().view(np.uint32), g.theta().view(np.uint32)), what
    finally:
        o.close()
    want = ru.accumulate(sweeps, regions[0], regions[1], c["edges"], D=D, P=P)
    got = g.regions()
    ru.assert_matches(got, want, what=what)
    return g, sweeps, regions, got, want


@pytest.mark.parametrize("name", ["k3", "depth", "k20_wide", "k4_mixed", "mv_c22", "compat_k4"])
def test_regions_match_checker(hml, name):
    """sweep_k, 2.9 10^5 blocks a sweep (more chunks than the scan has pieces), sweep_wide, a scheme with M, S, P and D tokens,
    D = 2, the reference-compatible mode"""
    c = bc.CASES[name]
    g, sweeps, regions, got, want = run_case(hml, c, what=name)
    start, end, edges = g.get_regions()
    assert np.array_equal(start, regions[0]) and np.array_equal(end, regions[1]) and np.array_equal(edges, np.asarray(c["edges"], np.float32))
    assert got["inband"].shape == (len(start), c["D"] * (len(c["edges"]) + 1))
    if name == "depth":
        assert max(len(s[1]) for s in sweeps) > 256 * 1024
    # something to find (tests/test_regions_cpu.py has more): whole regions and cut ones, and the duplicate carries the same sums twice
    N = want["N"]
    assert np.any(want["whole"] == N) and np.any(want["whole"] < N) and want["inband"].any(), name
    dup = np.flatnonzero((regions[0] == c["T"] // 3) & (regions[1] == c["T"] // 2))
    assert len(dup) == 2 and all(np.array_equal(got[k][..., dup[0]], got[k][..., dup[1]]) for k in ("whole", "breaks_sum", "breaks_sq") + DOUBLES)
    s = hml.regions_summary(got)
    assert np.allclose(s["p_whole"], want["whole"].astype(np.float64) / N, rtol=0, atol=0)
    assert np.all(s["level_sd"] >= 0) and s["p_inband"].shape == got["inband"].shape


@pytest.mark.parametrize("T", sorted(ru.EDGE_B))
def test_regions_at_chunk_edges(hml, T):
    """every position a block (the trace times 1024): B = 2, the wavefront width - 1, + 0, + 1, the chunk length - 1, + 0, + 1,
    and four chunks with the last one short of a block or full - with every region of the short traces and, on the longer ones,
    regions that begin and end around the chunk edges"""
    c = ru.edge_case(T)
    g, sweeps, regions, got, want = run_case(hml, c, what="T = %d" % T, regions=ru.edge_regions(T))
    assert all(len(s[1]) == ru.EDGE_B[T] for s in sweeps)
    assert want["breaks_sum"].max() > 0


def test_regions_without_edges(hml):
    """no edges: no band columns, everything else as with them"""
    c = dict(bc.CASES["k3"], T=50000, trace=lambda: ol.trace(50000, 3, 7), seed=11, scheme=[("F", 12, 2)], edges=())
    g, sweeps, regions, got, want = run_case(hml, c, what="no edges")
    assert got["inband"].shape == (len(regions[0]), 0) and got["N"] == 6


def test_regions_thinning_on_one_chain(hml):
    """thinning 1, 2, 3 and 7 in the tokens of one chain"""
    c = dict(bc.CASES["k3"], T=50000, trace=lambda: ol.trace(50000, 3, 7), seed=11,
             scheme=[("F", 6, 1), ("F", 8, 2), ("F", 9, 3), ("F", 15, 7)])
    g, sweeps, regions, got, want = run_case(hml, c, what="thinning")
    assert got["N"] == 6 + 4 + 3 + 2


def test_regions_off_and_on(hml):
    """n = 0 in the middle of a scheme, then the same regions again: only the sweeps recorded while on are counted; other regions
    or edges after a recorded sweep are refused, before one they are accepted"""
    c = dict(bc.CASES["k3"], T=50000, trace=lambda: ol.trace(50000, 3, 7), seed=12, scheme=[("F", 6, 1), ("F", 4, 1), ("F", 6, 2)])
    o = bc.checker(c)
    sweeps = bc.checker_sweeps(o, c["scheme"], recording=[True, False, True])
    o.close()
    regions = ru.standard_regions(c["T"], sweeps[-1], seed=2)
    other = (regions[0][:10].copy(), regions[1][:10].copy())
    g = gpu_chain(hml, c, regions=other, edges=(0.25,))
    g.regions()                                             # (the buffers of these regions exist now, and hold nothing)
    g.set_regions(*regions, c["edges"])                     # before a recorded sweep: free
    gpu_token(g, c["scheme"][0])
    g.set_regions((), ())
    gpu_token(g, c["scheme"][1])
    assert g.regions()["N"] == 6
    g.set_regions(*regions, c["edges"])                     # the same bits: on again
    gpu_token(g, c["scheme"][2])
    g.sync()
    got = g.regions()
    assert got["N"] == 6 + 3 == len(sweeps) and g.recorded_sweeps() == 6 + 4 + 3
    ru.assert_matches(got, ru.accumulate(sweeps, regions[0], regions[1], c["edges"]), what="off and on")
    moved = regions[1].copy()
    moved[np.flatnonzero(regions[1] - regions[0] >= 2)[0]] -= 1
    for bad in ((regions[0], moved, c["edges"]), (regions[0][:-1], regions[1][:-1], c["edges"]), (regions[0], regions[1], (-0.5,)),
                (regions[0], regions[1], ())):
        with pytest.raises(hml.HmlError) as e:
            g.set_regions(*bad)
        assert e.value.code == 1 and "cannot be changed" in str(e.value), bad[2]
    for bad, message in ((([5], [5], ()), "does not lie inside"), (([5], [c["T"] + 1], ()), "does not lie inside"),
                         (([0], [5], (0.5, -0.5)), "strictly ascending"), (([0], [5], (float("nan"),)), "finite"),
                         (([0], [5], tuple(range(32))), "1 to 31 edges")):
        with pytest.raises(hml.HmlError) as e:
            g.set_regions(*bad)
        assert e.value.code == 1 and message in str(e.value), (bad, str(e.value))
    assert same_bits(g.regions(), got)


def test_regions_given_before_the_observations(hml):
    """regions set on a fresh context are compared with T by the first recorded sweep"""
    x = ol.trace(20000, 3, 7)
    for end, ok in ((20000, True), (20001, False)):
        g = hml.Chain(device=0, seed=3)
        g.set_regions([0, 100], [50, end], (-0.5, 0.5))
        g.load(x)
        g.set_model(3, g.autoprior(0.2, 0.9))
        g.sample_prior()
        g.iterate("F", 3, 0)
        if ok:
            g.iterate("F", 2, 1)
            assert g.regions()["N"] == 2
        else:
            with pytest.raises(hml.HmlError) as e:
                g.iterate("F", 2, 1)
            assert e.value.code == 1 and "does not lie inside the 20000 positions" in str(e.value)
        g.close()


def test_regions_survive_buffer_growth(hml):
    """a block capacity far below what the sweeps need: the chain halts, hml_settle grows its buffers and runs the sweeps again -
    the same bits as with room from the start"""
    c = dict(bc.CASES["k3"], seed=8, scheme=[("M", 4, 1), ("F", 16, 2)])
    o = bc.checker(c)
    sweeps = bc.checker_sweeps(o, c["scheme"])
    o.close()
    regions = ru.standard_regions(c["T"], sweeps[-1], seed=3)
    g0 = gpu_run(gpu_chain(hml, c, regions=regions), c["scheme"])
    g1 = gpu_run(gpu_chain(hml, c, regions=regions, options=(("max_blocks", 64),)), c["scheme"])
    assert g0.stats()["buffer_growths"] == 0 and g1.stats()["buffer_growths"] > 0
    ref, got = g0.regions(), g1.regions()
    assert got["N"] == ref["N"] == 12 and same_bits(ref, got)
    ru.assert_matches(got, ru.accumulate(sweeps, regions[0], regions[1], c["edges"]), what="max_blocks 64")


def test_regions_iterate_many_equals_iterate_bit_for_bit(hml):
    """three chains attached to one trace through hml_iterate_many (the kernels run per chain behind the batch's parameter
    kernels): each chain's sums are those of the same chain alone under hml_iterate, bit for bit - and the checker's"""
    c = dict(bc.CASES["k5"], seed=21, scheme=[("F", 12, 0), ("F", 18, 3)])
    o = bc.checker(c)
    regions = ru.standard_regions(c["T"], bc.checker_sweeps(o, c["scheme"])[-1], seed=4)
    o.close()
    alone = []
    for k in range(3):
        g = gpu_run(gpu_chain(hml, c, chain=k, regions=regions), c["scheme"])
        alone.append(g.regions())
        g.close()
    first = gpu_chain(hml, c, chain=0, regions=regions)
    chains = [first] + [gpu_chain(hml, c, chain=k, attach=first, regions=regions) for k in (1, 2)]
    for g in chains:
        g.sample_prior()
        g._pending_prior = False
    for m, n, t in c["scheme"]:
        hml.iterate_many(chains, m, n, t)
    for k, g in enumerate(chains):
        g.sync()
        got = g.regions()
        assert got["N"] == 6 and same_bits(got, alone[k]), k
        o = bc.checker(c, chain=k)
        ru.assert_matches(got, ru.accumulate(bc.checker_sweeps(o, c["scheme"]), regions[0], regions[1], c["edges"]), what="iterate_many chain %d" % k)
        o.close()


def test_regions_merge_and_add(hml):
    """hml_regions_merge of two chains = the helper fed both chains' sweeps in the integers and dst + src in ONE addition, bit
    for bit, in the doubles; the source is unchanged and the destination records on; hml_regions_add with raw values makes
    breaks_sq saturate and stay there; mismatched regions, edges or T are refused"""
    c = dict(bc.CASES["k4_mixed"], T=80000, trace=lambda: ol.trace(80000, 4, 7))
    cA = dict(c, seed=13, scheme=[("F", 20, 2)])
    cB = dict(c, seed=14, scheme=[("M", 5, 0), ("F", 12, 1)])
    oA, oB = bc.checker(cA), bc.checker(cB, chain=1)
    sweepsA, sweepsB = bc.checker_sweeps(oA, cA["scheme"]), bc.checker_sweeps(oB, cB["scheme"])
    oA.close()
    oB.close()
    regions = ru.standard_regions(c["T"], sweepsA[-1], seed=5)
    a = gpu_run(gpu_chain(hml, cA, regions=regions), cA["scheme"])
    b = gpu_run(gpu_chain(hml, cB, chain=1, regions=regions), cB["scheme"])
    ra, rb = a.regions(), b.regions()
    a.regions_merge(b)
    got = a.regions()
    want = ru.accumulate(sweepsA + sweepsB, regions[0], regions[1], c["edges"])
    assert got["N"] == 22 == want["N"]
    for k in ("whole", "breaks_sum", "breaks_sq", "inband"):
        assert np.array_equal(got[k], want[k]), k
    for k in DOUBLES:
        assert np.array_equal(got[k].view(np.uint64), (ra[k] + rb[k]).view(np.uint64)), k
    assert same_bits(b.regions(), rb)                       # the source is unchanged
    a.iterate("F", 4, 2)                                    # the destination records on
    a.sync()
    assert a.regions()["N"] == 24
    # raw sums from anywhere: breaks_sq saturates and stays saturated
    huge = dict(rb, N=5, breaks_sq=np.full(len(regions[0]), 2 ** 64 - 3, np.uint64))
    huge["breaks_sq"][1] = 7
    before = a.regions()
    a.regions_add(huge)
    after = a.regions()
    assert after["N"] == before["N"] + 5
    assert np.array_equal(after["breaks_sq"], ru.sat_add(before["breaks_sq"], huge["breaks_sq"]))
    sat = after["breaks_sq"] == np.uint64(ru.U64_MAX)
    assert sat.any() and not sat[1] and after["breaks_sq"][1] == before["breaks_sq"][1] + 7
    assert np.array_equal(after["whole"], before["whole"] + rb["whole"]) and np.array_equal(after["inband"], before["inband"] + rb["inband"])
    for k in DOUBLES:
        assert np.array_equal(after[k].view(np.uint64), (before[k] + rb[k]).view(np.uint64)), k
    a.regions_add(dict(rb, N=0))
    again = a.regions()
    assert np.array_equal(again["breaks_sq"][sat], after["breaks_sq"][sat]) and again["N"] == after["N"]
    assert np.all(np.isnan(hml.regions_summary(again)["breaks_sd"][sat]))
    # refused: other regions (one position), other edges (one bit), other T, a source without regions
    moved = regions[1].copy()
    moved[np.flatnonzero(regions[1] - regions[0] >= 2)[0]] -= 1
    edges1 = np.asarray(c["edges"], np.float32).copy()
    edges1[0] = np.nextafter(edges1[0], np.float32(0))
    small = ru.standard_regions(40000, (np.array([0, 20000, 40000]),), seed=5)
    for bad in (gpu_run(gpu_chain(hml, cA, regions=(regions[0], moved)), [("F", 2, 1)]),
                gpu_run(gpu_chain(hml, cA, regions=regions, edges=edges1), [("F", 2, 1)]),
                gpu_run(gpu_chain(hml, dict(cA, T=40000), trace=lambda: ol.trace(40000, 4, 7), regions=small), [("F", 2, 1)]),
                gpu_run(gpu_chain(hml, cA), [("F", 2, 1)])):
        with pytest.raises(hml.HmlError) as e:
            a.regions_merge(bad)
        assert e.value.code == 1
        bad.close()
    assert same_bits(a.regions(), again)


def test_regions_off_by_default(hml):
    """no regions set: no launch of the family, the read-out refuses; with regions on, everything else is bit for bit what it
    is with them off"""
    c = dict(bc.CASES["k3"], T=50000, trace=lambda: ol.trace(50000, 3, 7), seed=5, scheme=[("F", 10, 1)])
    regions = ru.standard_regions(c["T"], (np.array([0, 25000, 50000]),), seed=6)
    kept = []
    for reg in (None, regions):
        g = gpu_chain(hml, c, regions=reg)
        g.set_level_recording(True)
        g.profile_enable(2)
        gpu_run(g, c["scheme"])
        assert g.recorded_sweeps() == 10 and g.profile_get("marginals")[1] == 10
        assert g.profile_get("regions")[1] == (0 if reg is None else 10)
        if reg is None:
            with pytest.raises(hml.HmlError) as e:
                g.regions()
            assert e.value.code == 1 and "hml_set_regions" in str(e.value)
        else:
            assert g.regions()["N"] == 10
        kept.append((g.blocks(), g.states(), g.theta().view(np.uint32), g.marginals_rle(), g.levels_rle()))
    a, b = kept
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert np.array_equal(a[3][0], b[3][0]) and np.array_equal(a[3][1], b[3][1])
    assert a[4][1] == b[4][1] and np.array_equal(a[4][0], b[4][0])
    assert np.array_equal(a[4][2].view(np.uint64), b[4][2].view(np.uint64)) and np.array_equal(a[4][3].view(np.uint64), b[4][3].view(np.uint64))
    # given, nothing recorded: zeros with N = 0
    g = gpu_chain(hml, c, regions=regions)
    gpu_run(g, [("F", 4, 0)])
    got = g.regions()
    assert got["N"] == 0 and not got["whole"].any() and not got["level_sum"].any() and not got["inband"].any()

"""The default path against the CPU checker in device mode at the sizes the benchmark quotes: 10^7 ... 10^8 positions,
up to 2.4*10^7 blocks a sweep, with no threshold forced - the weakly compressed sweep (rows / dense counts / state
kernels, refit rounds, checkpoints, flag-staged scan) switches on because the chain has 2^22 blocks, not because an
environment variable says so.  Everything is compared on bits after every `iterate` call: block starts, state
sequence, parameters, the count pass, the recorded marginals, the number of block updates; forward rows where the
probes are on.  There is no tolerance in this file and it sets no HML_* variable (it removes them all).
Reference behaviour under test: the whole sweep, src/HMM.hpp:99-121, src/StateSequence/ForwardBackward.hpp:65-211.

Each case's docstring records what an MI355X run showed (blocks after each call, repair counters), so a reader knows
which machinery the case exercised; the same figures and the wall times are in profiles/fullsize_checker_tests.txt."""
import time

import numpy as np
import pytest

from tests import fuzz_util
from tests import oracle_lib as ol
from tests.test_gpu_parity import bits, compare_state, make_pair, setup_model

pytestmark = pytest.mark.gpu

DENSE_MIN = 1 << 22      # hml_sweep_plan.h dense_min_blocks: the weakly compressed sweep from that many blocks on
MID_MIN = 1 << 18        # hml_sweep_plan.h mid_min_blocks: chunks of 8 from that many blocks on
TEXT_BELOW = 10 ** 6     # marginals are compared as text below that many segments, as arrays above
REPAIR = ("forward_refits", "forward_serial", "fused_fallbacks", "buffer_growths")


@pytest.fixture(autouse=True)
def no_switches(monkeypatch):
    """an outer environment must not move a threshold: every switch the library reads is removed"""
    for k in fuzz_util.ENV_KEYS:
        monkeypatch.delenv(k, raising=False)


@pytest.fixture(scope="module")
def c3_trace():
    return ol.trace(100_000_000, 5, 3)


@pytest.fixture(scope="module")
def c3u_trace():
    return ol.trace(10_000_000, 5, 3)


def dense_runs(dense):
    """maximal runs of equal columns of a (K, T) array: (start positions, (n, K) counts)"""
    K, T = dense.shape
    change = np.zeros(T, bool)
    change[0] = True
    for k in range(K):
        change[1:] |= dense[k, 1:] != dense[k, :-1]
    starts = np.flatnonzero(change)
    return starts, np.ascontiguousarray(dense[:, starts].T)


def merged_runs(seg, cnt, K):
    """the run-length form of the product (a segment per recorded block boundary; a column per state seen) as maximal
    runs of equal counts over all K states"""
    full = np.zeros((len(seg), K), np.int32)
    full[:, :cnt.shape[1]] = cnt
    starts = np.concatenate([[0], np.cumsum(seg.astype(np.int64))[:-1]])
    keep = np.ones(len(seg), bool)
    keep[1:] = (full[1:] != full[:-1]).any(axis=1)
    return starts[keep], full[keep]


def compare_marginals(hml, o, g, what):
    seg, cnt = g.marginals_rle()
    assert int(seg.sum()) == o.T, what
    if len(seg) < TEXT_BELOW:
        assert hml.marginals_text(seg, cnt) == o.text("marginals"), what
        return
    so, co = dense_runs(o.marginals_dense())
    sg, cg = merged_runs(seg, cnt, o.K)
    assert np.array_equal(so, sg), what
    assert np.array_equal(co, cg), what


def compare_counts(o, g, what):
    to, oo, so, qo, _ = o.counts()
    tg, og, sg, qg, _ = g.counts()
    assert np.array_equal(to, tg), what
    assert np.array_equal(oo, og), what
    assert np.array_equal(bits(so), bits(sg)) and np.array_equal(bits(qo), bits(qg)), what
    return og


def compare_all(hml, o, g, what, recorded, probes=False):
    compare_state(o, g, what)
    occ = compare_counts(o, g, what)
    if probes:
        assert np.array_equal(bits(o.forward_rows()), bits(g.forward_rows())), what
    compare_marginals(hml, o, g, what)
    assert g.recorded_sweeps() == recorded == ol.load().orc_n_recorded(o.h), what
    assert g.stats()["block_updates"] == o.total_blocks(), what
    return occ


def split_scheme(sweeps, thin):
    """`F sweeps thin` (thin >= 2) with the first two sweeps as calls of their own, recording the very sweeps the one
    call would (thin, 2 thin, ...): a failure names the sweep, and the first sweep (no block-count hint yet) is checked
    apart from the steady ones.  Sweeps that are not recorded are the ones the captured graph replays."""
    assert 2 <= thin <= sweeps
    calls = [("F", 1, 0), ("F", 1, 1 if thin == 2 else 0)]
    done = 2
    if thin > 2:
        calls.append(("F", thin - 2, thin - 2))
        done = thin
    if sweeps > done:
        calls.append(("F", sweeps - done, thin))
    return calls


def start_pair(hml, x, K, seed, chain=0, probes=False, **kw):
    _, o, g = make_pair(hml, x.size, K, 0, seed, chain=chain, x=x, **kw)
    try:
        setup_model(o, g, K)
        o.token("F")
        g.sample_prior()
        o.set_record(marginals=True)
        if probes:
            o.set_probes(True)
            g.enable_probes(True)
    except BaseException:
        g.close()
        o.close()
        raise
    return o, g


def run_case(hml, name, o, g, scheme, probes=False, floor=None):
    """the scheme call by call on both sides, everything compared after every call; returns the checker's block count
    after each call and the product's counters.  floor[i]: the least number of blocks the checker must have after call i."""
    counts, recorded, t_chk, t_gpu, t0 = [], 0, 0.0, 0.0, time.time()
    occ = None
    for i, (m, n, thin) in enumerate(scheme):
        t = time.time()
        o.iterate(m, n, thin)
        t_chk += time.time() - t
        t = time.time()
        g.iterate(m, n, thin)
        g.sync()
        t_gpu += time.time() - t
        recorded += n // thin if thin else 0
        B = int(o.num_blocks())
        counts.append(B)
        if floor is not None and i < len(floor) and floor[i] is not None:
            assert B >= floor[i], (name, "call", i, "blocks", B, counts)
        occ = compare_all(hml, o, g, (name, "call", i, (m, n, thin), "blocks", B), recorded, probes)
    st = g.stats()
    print("\n[fullsize-checker] %s: blocks after each call %s; %s; checker sweeps %.2f s, GPU sweeps %.3f s, case %.1f s" % (
        name, counts, ", ".join("%s %d" % (k, st[k]) for k in REPAIR), t_chk, t_gpu, time.time() - t0))
    return counts, st, occ


def test_c3_full_size(hml, c3_trace):
    """BASELINE config 3 at full size: 10^8 Gaussian positions, 5 states, 12 sweeps, thinning 4 (as F 1 0, F 1 0, F 2 2, F 8 4).
    Occupancies beyond 2^24: the exact-integer count regime.
    MI355X: 229 955, 156 194, 176 134, 176 256 blocks after the four calls; forward_refits 0, forward_serial 0,
    fused_fallbacks 0, buffer_growths 0 (a settled 5-state chain needs no repair: the fused sparse sweep as benchmarked)."""
    o, g = start_pair(hml, c3_trace, 5, seed=1)
    try:
        counts, st, occ = run_case(hml, "c3", o, g, split_scheme(12, 4))
        assert int(occ.max()) > (1 << 24)
        assert 1.2e5 < counts[-1] < 2.6e5
    finally:
        g.close()
        o.close()


def test_c4_full_size(hml):
    """BASELINE config 4 at full size: 10^8 Gaussian positions of 10 levels, 10 states, chain 3 of its seed, 8 sweeps,
    thinning 4 (as F 1 0, F 1 0, F 2 2, F 4 4), probes on: forward rows compared - 10 states keep twin states while
    the chain burns in, so the repair path works here.
    MI355X: 295 602, 214 804, 204 626, 197 906 blocks after the four calls; forward_refits 7, forward_serial 0,
    fused_fallbacks 0, buffer_growths 0."""
    x = ol.trace(100_000_000, 10, 4)
    o, g = start_pair(hml, x, 10, seed=1, chain=3, probes=True)
    try:
        counts, st, occ = run_case(hml, "c4", o, g, split_scheme(8, 4), probes=True)
        assert st["forward_refits"] > 0, st      # (the repaired chunks' rows were among those compared)
    finally:
        g.close()
        o.close()


def test_c3u_natural_threshold(hml, c3u_trace):
    """Config 3 uncompressed (weights x 1e9: every position a block) at 10^7 positions: 2^22 blocks reached by the
    chain itself, which is what puts the sweep on the weakly compressed path.  `F 3 1` as F 1 0, F 1 0, F 1 1; probes on
    (200 MB of forward rows a side).
    MI355X: 10^7 blocks in every sweep; forward_refits 28, forward_serial 0, fused_fallbacks 0, buffer_growths 0."""
    o, g = start_pair(hml, c3u_trace, 5, seed=1, probes=True, weight_mult=1e9)
    try:
        run_case(hml, "c3u", o, g, [("F", 1, 0), ("F", 1, 0), ("F", 1, 1)], probes=True, floor=[DENSE_MIN] * 3)
    finally:
        g.close()
        o.close()


@pytest.mark.parametrize("seed", [7, 1])
def test_c5_prefix(hml, seed):
    """A 2.5*10^7 prefix of BASELINE config 5 (integer read depths, 5 states): four single sweeps, then F 2 1.  The
    first four sweeps stay at or above 2^22 blocks on the checker; chain seed 7 falls through several chunk-length
    picks on the way, chain seed 1 stays at 9.3*10^6.  The marginals of the last call are compared as arrays.
    MI355X, blocks after the five calls - seed 7: 24 355 329, 15 540 460, 7 070 365, 5 276 085, 5 106 455 (sweeps 5-6 stay
    above 2^22: no natural crossing here, that is the next case); forward_refits 0.  Seed 1: 23 107 793, 11 764 446,
    9 317 540, 9 318 466, 14 097 615 (it grows again); forward_refits 58.  Both: forward_serial 0, fused_fallbacks 0,
    buffer_growths 0."""
    x = ol.synth_depth(25_000_000, depth=15.0, ln_sigma=0.15, seed=5)
    o, g = start_pair(hml, x, 5, seed=seed)
    try:
        run_case(hml, "c5_seed%d" % seed, o, g, [("F", 1, 0)] * 4 + [("F", 2, 1)],
                 floor=[DENSE_MIN] * 4)
    finally:
        g.close()
        o.close()


@pytest.mark.parametrize("mult", [2.0, 3.0])
def test_crossing_the_thresholds(hml, c3u_trace, mult):
    """One chain through dense -> mid -> sparse with nothing forced: the geometry of a sweep follows the previous
    sweep's block count, so each hand-over runs with a hint from the other side of the threshold.  Six single sweeps:
    four unrecorded ones (those a captured graph replays, captured anew at each hand-over), two recorded ones.
    MI355X, blocks after the six calls - weights x 2: 4 860 709, 732 871, 202 884, 154 749, 154 280, 153 968; weights x 3:
    6 753 170, 4 043 761, 2 486 967, 1 641 211, 1 567 395, 1 559 284.  Both: forward_refits 0, forward_serial 0,
    fused_fallbacks 0, buffer_growths 0."""
    o, g = start_pair(hml, c3u_trace, 5, seed=7, weight_mult=mult)
    try:
        counts, st, occ = run_case(hml, "crossing_x%g" % mult, o, g, [("F", 1, 0)] * 4 + [("F", 1, 1)] * 2,
                                   floor=[DENSE_MIN])
        # the checker's counts bracket the thresholds, so the case cannot silently stop crossing
        assert any(MID_MIN <= b < DENSE_MIN for b in counts[1:]), counts
        if mult == 2.0:
            assert counts[-1] < MID_MIN, counts
    finally:
        g.close()
        o.close()


def test_wide_path_above_dense_threshold(hml):
    """More than 16 states (a state a lane / a chunk a lane, hml_k_wide_lanes.h) at 5*10^6 blocks a sweep: `F 2 1`
    as F 1 0 (graph-eligible), F 1 1.  Whether the graph is replayed or captured again there, the results are the checker's.
    MI355X: 5*10^6 blocks in both sweeps; forward_refits 185, forward_serial 0, fused_fallbacks 0, buffer_growths 0."""
    x = ol.trace(5_000_000, 5, 3)
    o, g = start_pair(hml, x, 20, seed=1, weight_mult=1e9)
    try:
        run_case(hml, "wide_k20", o, g, [("F", 1, 0), ("F", 1, 1)], floor=[DENSE_MIN] * 2)
    finally:
        g.close()
        o.close()


def test_three_chains_in_one_set_of_launches_at_c3(hml, c3_trace):
    """Three chains of one seed attached to one construction and swept through hml_iterate_many (the many-chain block
    and forward kernels at 763 tiles), each against the checker's chain of the same (seed, chain) run alone, one after another.  `F 6 2` as F 1 0, F 1 1, F 4 2.
    MI355X, blocks after the three calls - chain 0: 229 955, 156 194, 176 200; chain 1: 309 666, 175 160, 176 159; chain 2:
    642 455, 181 968, 189 108.  All three: forward_refits 0, forward_serial 0, fused_fallbacks 0, buffer_growths 0."""
    x, K, seed = c3_trace, 5, 1
    scheme = split_scheme(6, 2)
    gs, snaps, prior = [], [], []
    try:
        for chain in range(3):
            g = hml.Chain(device=0, seed=seed, chain_id=chain)
            gs.append(g)
            if chain:
                g.attach(gs[0])
            else:
                g.load(x)
            prior.append(g.autoprior(0.2, 0.9))
            g.set_model(K, prior[-1])
            g.sample_prior()
        t = time.time()
        for m, n, thin in scheme:
            hml.iterate_many(gs, m, n, thin)
            snap = []
            for g in gs:
                g.sync()
                snap.append({"blocks": g.blocks(), "states": g.states(), "theta": g.theta(), "trans": g.transitions(),
                             "counts": g.counts(), "marg": g.marginals_rle(), "recorded": g.recorded_sweeps(),
                             "updates": g.stats()["block_updates"]})
            snaps.append(snap)
        t_gpu = time.time() - t
        stats = [g.stats() for g in gs]
    finally:
        for g in reversed(gs):
            g.close()
    t = time.time()
    for chain in range(3):
        o = ol.OracleChain(K=K, seed=seed, chain=chain, rng=ol.RNG_CTR, math=ol.MATH_DEV, reduce=ol.REDUCE_DEV)
        try:
            o.load(x)
            assert np.array_equal(bits(o.autoprior()), bits(prior[chain]))
            o.init_model()
            o.token("F")
            o.set_record(marginals=True)
            counts, recorded = [], 0
            for i, (m, n, thin) in enumerate(scheme):
                o.iterate(m, n, thin)
                recorded += n // thin if thin else 0
                s = snaps[i][chain]
                what = ("chain", chain, "call", i, (m, n, thin))
                counts.append(int(o.num_blocks()))
                assert np.array_equal(o.blocks(), s["blocks"]), what
                assert np.array_equal(o.states(), s["states"]), what
                assert np.array_equal(bits(o.theta()), bits(s["theta"])), what
                Ao, pio = o.transitions()
                assert np.array_equal(bits(Ao), bits(s["trans"][0])) and np.array_equal(bits(pio), bits(s["trans"][1])), what
                to, oo, so, qo, _ = o.counts()
                tg, og, sg, qg, _ = s["counts"]
                assert np.array_equal(to, tg) and np.array_equal(oo, og), what
                assert np.array_equal(bits(so), bits(sg)) and np.array_equal(bits(qo), bits(qg)), what
                assert len(s["marg"][0]) < TEXT_BELOW, what
                assert hml.marginals_text(*s["marg"]) == o.text("marginals"), what
                assert s["recorded"] == recorded == ol.load().orc_n_recorded(o.h), what
                assert s["updates"] == o.total_blocks(), what
            print("\n[fullsize-checker] many chain %d: blocks after each call %s; %s" % (
                chain, counts, ", ".join("%s %d" % (k, stats[chain][k]) for k in REPAIR)))
        finally:
            o.close()
    print("[fullsize-checker] many: checker %.1f s, GPU sweeps and read-backs %.2f s" % (time.time() - t, t_gpu))

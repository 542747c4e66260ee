"""The pairwise read-outs of the smoothing on the device (hml_posterior_breaks, hml_posterior_regions, hml_posterior_pair_terms,
include/hml.h) against the restatement for one host thread, tests/fixtures/pairs_ref_main.cpp over
hammlet_amd/csrc/hml_pairs_ref.h, which is fed the GPU's own block_stats(), blocks(), theta() and transitions().  Every double
is compared as its 64-bit word and every fixed-point value as an integer: p, r, pfx, cost, mass, the break list, and the
regions' doubles and raw integers.  There is no tolerance anywhere in this file except in the consistency check with the
E-step, which compares two different sums."""
import gc
import numpy as np
import pytest

from tests import hostile_inputs as hi
from tests import oracle_lib as ol
from tests import pairs_util as pz
from tests import posterior_util as pu

pytestmark = pytest.mark.gpu

# the sizes at which the device code takes another path
SCAN_CHUNK = 1024          # entries a chunk of the three-phase scan (HML_SCAN_CHUNK)
COUNT_CHUNK = 256          # blocks a workgroup of the break list's count and scatter
SCAN_PIECES = 1024         # chunk totals the scan's middle phase takes one a thread: above SCAN_PIECES chunks a thread adds several
N_RANDOM = 2000


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return pz.build_programs(tmp_path_factory.mktemp("pairs_ref"), sanitized=False)["plain"]


def chain(hml, x, K, seed=3, sweeps=3, options=(), dims=None, self_trans=True, every_position=False):
    g = hml.Chain(device=0, seed=seed)
    for name, value in options:
        g.set_option(name, value)
    if dims:
        g.set_dimensions(*dims)
    g.load(x)
    if every_position:
        g.scale_weights(1e9)
    g.set_model(K, g.autoprior(0.2, 0.9), self_trans=self_trans)
    g.sample_prior()
    if sweeps:
        g.iterate("F", sweeps, 0)
        g.sync()
    return g


def terms_words(t):
    return dict(p=pu.words(t["p"]), r=pu.words(t["r"]), pfx=t["pfx"].ravel(), cost=t["cost"].ravel(), mass=t["mass"].ravel())


def check_breaks(g, want, starts, what=None):
    """the break list under min_prob 0, 0.5, 1 and 2 against the restatement's p"""
    p = want["p"].view(np.float64)
    B = len(p)
    for min_prob in (0.0, 0.5, 1.0, 2.0):
        got = g.posterior_breaks(min_prob)
        keep = np.flatnonzero(p[1:] >= min_prob) + 1
        assert np.array_equal(got["pos"], np.asarray(starts)[keep].astype(np.uint32)), (what, min_prob)
        assert np.array_equal(pu.words(got["prob"]), want["p"][keep]), (what, min_prob)
        assert pu.words([got["expected_breaks"]])[0] == pu.words([float(want["total"]) * 2.0 ** -32])[0], (what, min_prob)
        assert got["pair_degenerate"] == want["pair_degenerate"], (what, min_prob)
        if min_prob == 0.0:
            assert len(got["pos"]) == B - 1, what
        if min_prob == 2.0:
            assert len(got["pos"]) == 0, what


def check(hml, program, g, self_trans=True, what=None, n_random=N_RANDOM):
    """the terms, the break lists and the regions equal the restatement's words"""
    case = pu.chain_case(g, self_trans)
    rng = np.random.default_rng(g.num_blocks())
    start, end = pz.edge_regions(case["starts"], rng, n_random)
    want = pz.run_program(program, case, start, end)
    got = terms_words(g.posterior_pair_terms())
    for key in pz.WORD_KEYS:
        assert np.array_equal(got[key], want[key].ravel()), (what, key)
    check_breaks(g, want, case["starts"], what)
    r = g.posterior_regions(start, end, raw=True)
    assert r["pair_degenerate"] == want["pair_degenerate"], what
    pz.same_regions(pz.region_words(r), want, what)
    plain = g.posterior_regions(start, end)
    assert "raw" not in plain and np.array_equal(pu.words(plain["share"]), pu.words(r["share"]))
    # n = 0 succeeds; regions without a position, or past the end, are refused
    empty = g.posterior_regions([], [])
    assert empty["whole"].shape == (0,) and empty["share"].shape == (0, g.K) and empty["pair_degenerate"] == want["pair_degenerate"]
    T = g.T
    for a, e in [(1, 1), (2, 1), (0, T + 1), (T, T + 1)]:
        with pytest.raises(hml.HmlError) as err:
            g.posterior_regions([0, a], [1, e])
        assert err.value.code == 1 and "region 1" in str(err.value), (what, a, e)
    return want


def test_min_prob_that_is_no_number_is_refused(hml):
    g = chain(hml, ol.trace(100, 3, 2), 2)
    with pytest.raises(hml.HmlError) as err:
        g.posterior_breaks(float("nan"))
    assert err.value.code == 1 and "not a number" in str(err.value)


@pytest.mark.parametrize("T", [2, 3, 16, 65])
def test_tiny_traces(hml, program, T):
    g = chain(hml, ol.trace(1000, 3, 2)[:T].copy(), 2, seed=12, sweeps=10)
    want = check(hml, program, g, what=T, n_random=50)
    assert want["pair_degenerate"] == 0


def test_one_block(hml, program):
    g = hml.Chain(device=0, seed=12)
    g.load(np.array([0.3], np.float32))
    g.set_model(2, np.array([2.0, 1.0, 0.0, 1.0], np.float32))
    g.sample_prior()
    g.create_blocks(1.0)
    assert g.num_blocks() == 1
    check(hml, program, g, what="B = 1", n_random=0)
    got = g.posterior_breaks()
    assert len(got["pos"]) == 0 and got["expected_breaks"] == 0.0
    r = g.posterior_regions([0], [1])
    assert r["expected_breaks"][0] == 0.0 and r["whole"][0] == pytest.approx(1.0, abs=1e-15)


@pytest.mark.parametrize("B", [COUNT_CHUNK - 1, COUNT_CHUNK, COUNT_CHUNK + 1, SCAN_CHUNK - 1, SCAN_CHUNK, SCAN_CHUNK + 1, 4095, 4096, 4097, 70000])
def test_every_position_a_block(hml, program, B):
    """both sides of the break list's workgroup (256 blocks) and of the scan's chunk (1024 entries), the smoothing's own
    64 x 64, and 70 000: 69 chunks a row, 274 workgroups of the break list"""
    g = chain(hml, ol.trace(B, 5, 4), 5, every_position=True)
    assert g.num_blocks() == B
    want = check(hml, program, g, what=B)
    assert want["pair_degenerate"] == 0


def test_more_chunks_than_the_chunk_sum_row_is_wide(hml):
    """B = 1024 x 1024 + 1025: 1026 chunks a row, so a thread of the scan's middle phase adds two chunk totals, and 4101
    workgroups of the break list, whose counts are scanned the same way.  The restatement's text would take minutes at this size;
    integers need none: the raw words of the regions are differences of plain cumulative sums of the device's own terms, which
    the smaller shapes above tie to the restatement"""
    B = SCAN_CHUNK * SCAN_PIECES + SCAN_CHUNK + 1
    g = chain(hml, ol.trace(B, 2, 4), 2, sweeps=1, every_position=True)
    assert g.num_blocks() == B
    t = g.posterior_pair_terms()
    N, C, G = np.cumsum(t["pfx"]), np.cumsum(t["cost"], axis=0), np.cumsum(t["mass"], axis=0)
    rng = np.random.default_rng(5)
    a = np.concatenate([[0, 0, B - 1], rng.integers(0, B, 3000)])
    e = np.concatenate([[1, B, B], np.minimum(a[3:] + rng.integers(1, 3 * SCAN_CHUNK * SCAN_PIECES // 2, 3000), B)])
    r = g.posterior_regions(a, e, raw=True)["raw"]
    ba, be = a, e - 1                                     # (a block a position)
    assert np.array_equal(r[:, 0], N[be] - N[ba])
    assert np.array_equal(r[:, 1:3], C[be] - C[ba])
    before = np.where(ba[:, None] > 0, G[np.maximum(ba, 1) - 1], 0)
    assert np.array_equal(r[:, 3:5], G[be] - before)
    got = g.posterior_breaks(0.5)
    keep = np.flatnonzero(t["p"][1:] >= 0.5) + 1
    assert np.array_equal(got["pos"], keep.astype(np.uint32)) and np.array_equal(pu.words(got["prob"]), pu.words(t["p"][keep]))
    assert got["expected_breaks"] == float(N[-1]) * 2.0 ** -32


@pytest.mark.parametrize("K", [2, 8, 9, 16, 17, 64])
def test_numbers_of_states(hml, program, K):
    """both sides of the kernel's two thresholds (8 and 16 states)"""
    B = 4100 if K <= 17 else 1500          # (the restatement's text grows with B K: more than one chunk of the scan either way)
    g = chain(hml, ol.trace(B, min(K, 5), 7), K, every_position=True)
    assert g.num_blocks() == B
    check(hml, program, g, what=K)


def test_blocks_of_many_positions(hml, program):
    g = chain(hml, ol.trace(30000, 5, 8), 5)
    assert g.num_blocks() < 30000
    check(hml, program, g)
    r = g.posterior_regions([0], [30000])
    assert abs(r["share"][0].sum() - 1.0) <= 5 * 2.0 ** -33
    assert r["expected_breaks"][0] == g.posterior_breaks()["expected_breaks"]


def test_two_dimensions_two_parameters(hml, program):
    T = 4096
    x = np.stack([ol.trace(T, 3, 1), ol.trace(T, 3, 2)], axis=1).reshape(-1)
    for every in (False, True):
        g = chain(hml, x, 4, dims=(2, 2), every_position=every)
        check(hml, program, g, what=every)


@pytest.mark.parametrize("name", hi.family("ties"))
def test_integer_data_full_of_ties(hml, program, name):
    fn, K, _ = hi.INPUTS[name]
    g = chain(hml, hi.data(name)[:20000], K, seed=hi.SEED[name], sweeps=5)
    check(hml, program, g, what=name)


def test_self_transitions_off(hml, program):
    g = chain(hml, ol.trace(20000, 3, 5), 3, self_trans=False)
    check(hml, program, g, self_trans=False)


def test_compat_context(hml, program):
    g = chain(hml, ol.trace(20000, 3, 6), 3, options=[("compat", 1)], sweeps=5)
    g.create_blocks(g.threshold())
    check(hml, program, g, what="compat")


def test_zeros_in_A_and_pi(hml, program):
    """(the diagonal of A stays positive, as the smoothing's test explains)"""
    g = chain(hml, ol.trace(20000, 3, 9), 3, every_position=True)
    A = np.array([[0.5, 0.5, 0.0], [0.0, 0.5, 0.5], [0.75, 0.0, 0.25]], np.float32)
    g.set_parameters(np.array([-1.0, 0.05, 0.0, 0.05, 1.0, 0.05], np.float32), A, np.array([0.0, 1.0, 0.0], np.float32))
    want = check(hml, program, g)
    assert want["pair_degenerate"] == 0


def test_a_zero_on_the_diagonal_caps_the_cost(hml, program):
    g = chain(hml, ol.trace(2000, 3, 9), 3, every_position=True, self_trans=False)
    A = np.array([[0.0, 0.5, 0.5], [0.25, 0.5, 0.25], [0.25, 0.25, 0.5]], np.float32)
    g.set_parameters(np.array([-1.0, 0.5, 0.0, 0.5, 1.0, 0.5], np.float32), A, np.array([0.25, 0.5, 0.25], np.float32))
    check(hml, program, g, self_trans=False)
    t = g.posterior_pair_terms()
    assert np.all(t["cost"][1:, 0] == pz.CAP) and np.all(t["r"][1:, 0] == 0.0)
    r = g.posterior_regions([0, 5], [2, 2000])
    assert np.all(r["whole_state"][:, 0] == 0.0)


def test_a_block_no_path_reaches(hml, program):
    x = np.random.default_rng(2).normal(0, 0.3, 300).astype(np.float32)
    x[1:3] += 40.0
    g = chain(hml, x, 3, sweeps=1, every_position=True, self_trans=False)
    A = np.array([[0.5, 0.25, 0.25], [1.0, 0.0, 0.0], [0.25, 0.25, 0.5]], np.float32)
    g.set_parameters(np.array([0.0, 1.0, 0.0, 1.0, 40.0, 1.0], np.float32), A, np.array([0.0, 1.0, 0.0], np.float32))
    assert g.num_blocks() == 300
    want = check(hml, program, g, self_trans=False)
    assert want["pair_degenerate"] >= 1
    t = g.posterior_pair_terms()
    r = g.posterior_regions(np.arange(0, 299), np.arange(1, 300) + 1)
    for a in (t["p"], t["r"], r["whole"], r["whole_state"], r["expected_breaks"], r["share"]):
        assert not np.isnan(a).any()


# ---------------------------------------------------------------------------------------------- geometry is invisible
def test_geometry_is_invisible(hml, program):
    """the decode's weakly separated trace: the words do not move under geometries of the smoothing pass that make the repair
    and the single lane run"""
    rng = np.random.default_rng(17)
    B = 20000
    st = np.cumsum(rng.random(B) < 0.01) % 5
    x = (0.5 * st + rng.normal(0, 1, B)).astype(np.float32)
    g = chain(hml, x, 5, sweeps=1, every_position=True)
    A = np.full((5, 5), 0.0025, np.float32)
    np.fill_diagonal(A, 0.99)
    mv = np.stack([0.5 * np.arange(5), np.ones(5)], 1).ravel().astype(np.float32)
    g.set_parameters(mv, A, np.full(5, 0.2, np.float32))
    assert g.num_blocks() == B
    check(hml, program, g, n_random=300)
    start, end = pz.edge_regions(g.blocks(), rng, 500)
    flat = lambda d: [np.asarray(v).tobytes() for v in d.values()]
    first = flat(g.posterior_pair_terms()) + flat(g.posterior_regions(start, end, raw=True)) + flat(g.posterior_breaks(0.5))
    seen_repair = seen_serial = False
    for W, L, rounds in [(1, 4, 0), (1, 64, 1), (4, 512, 8), (1024, 64, 8), (1, 512, 2)]:
        g.set_option("posterior_W", W)
        g.set_option("posterior_L", L)
        g.set_option("posterior_rounds", rounds)
        got = flat(g.posterior_pair_terms()) + flat(g.posterior_regions(start, end, raw=True)) + flat(g.posterior_breaks(0.5))
        assert got == first, (W, L, rounds)
        info = g.posterior_info()                 # the smoothing pass behind the last call
        assert info["W"] == W and info["L"] == L
        seen_repair |= info["stale_fwd"] > 0 and info["stale_bwd"] > 0
        seen_serial |= info["serial_chunks"] > 0
    assert seen_repair and seen_serial


# ---------------------------------------------------------------------------------------------- consistency with the E-step
def test_expected_breaks_agree_with_the_expected_counts(hml):
    """sum_b p_b = (B - 1) - trace(xi): two different sums of the same terms, within the 1e-9 of the CPU identity plus the
    list's own quantisation (B - 1) 2^-33"""
    g = chain(hml, ol.trace(30000, 5, 8), 5)
    B = g.num_blocks()
    got = g.posterior_breaks(0.0)
    xi = g.expected_counts()["xi"]
    assert abs(got["expected_breaks"] - ((B - 1) - np.trace(xi))) <= 1e-9 + (B - 1) * 2.0 ** -33
    assert abs(got["prob"].sum() - got["expected_breaks"]) <= 1e-9 + (B - 1) * 2.0 ** -33


# ---------------------------------------------------------------------------------------------- memory, side effects
def test_calls_keep_no_device_memory_and_survive_failed_allocations(hml):
    g = chain(hml, ol.trace(5000, 3, 3), 3, every_position=True)
    g.set_option("posterior_W", 1)      # (stale chunks: the repair kernels run too)
    rng = np.random.default_rng(1)
    start, end = pz.edge_regions(g.blocks(), rng, 100)
    gc.collect()      # (chains that earlier tests dropped without closing go first: the totals below are this test's alone)
    before = hml.device_memory_live()
    flat = lambda d: [np.asarray(v).tobytes() for v in d.values()]
    calls = {"posterior_breaks": lambda: g.posterior_breaks(0.25), "posterior_regions": lambda: g.posterior_regions(start, end, raw=True),
             "posterior_pair_terms": g.posterior_pair_terms}
    for name, call in calls.items():
        hml.debug_fail_allocation(10 ** 9)
        good = call()
        n_alloc = hml.debug_fail_allocation(0)
        assert n_alloc >= 5 and hml.device_memory_live() == before, name
        for n in range(1, n_alloc + 1):
            hml.debug_fail_allocation(n)
            with pytest.raises(hml.HmlError) as e:
                call()
            hml.debug_fail_allocation(0)
            assert e.value.code == 2 and "out of memory" in str(e.value), (name, n)
            assert hml.device_memory_live() == before, (name, n)
        assert flat(call()) == flat(good) and hml.device_memory_live() == before, name


def test_the_calls_leave_the_chain_alone(hml):
    x = ol.trace(40000, 3, 13)

    def run(call):
        g = chain(hml, x, 3, seed=5, sweeps=0)
        g.set_regions([0, 100], [50, 30000])      # a recording of the sampler's own regions goes on undisturbed
        g.iterate("F", 6, 2)
        if call:
            g.posterior_breaks(0.5)
            g.posterior_regions([0, 10, 10], [40000, 20, 20])
        g.iterate("F", 6, 2)
        if call:
            g.set_option("posterior_W", 1)
            g.posterior_pair_terms()
            g.posterior_regions([5], [6], raw=True)
        g.iterate("M", 2, 1)
        g.sync()
        seg, cnt = g.marginals_rle()
        rec = g.regions()
        return g.states(), g.theta(), g.transitions(), seg, cnt, g.blocks(), tuple(np.asarray(rec[k]) for k in sorted(rec))

    a, b = run(False), run(True)
    flat = lambda r: [np.asarray(v).tobytes() for part in r for v in (part if isinstance(part, tuple) else (part,))]
    assert flat(a) == flat(b)

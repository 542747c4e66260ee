"""EM from many starts on the device (hml_em_fit_many, hml_em_starts, hml_em_many_info, hml_set_em_batch_bytes, include/hml.h).
Member r of a batch is set_parameters(start r) + em_fit on the same chain, word for word: every case builds that twin and
compares the trace's 64-bit words, steps, reason, kept and the fitted floats' 32-bit words; for some members the restatement
for one host thread (tests/fixtures/em_ref_main.cpp in fit mode, fed the GPU's own blocks, statistics and the start) gives the
same.  There is no tolerance anywhere in this file."""
import gc
import numpy as np
import pytest

from tests import em_many_util as mu
from tests import em_util as eu
from tests import hostile_inputs as hi
from tests import oracle_lib as ol
from tests import posterior_util as pu
from tests.test_gpu_em import chain, prior

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return eu.build_programs(tmp_path_factory.mktemp("em_ref"), sanitized=False)["plain"]


def parameters(g):
    return [v.tobytes() for v in (g.theta(),) + tuple(g.transitions())]


def member_words(got, r):
    k = int(got["steps"][r])
    return dict(trace=pu.words(got["trace"][r, :k + 1]), steps=k, reason=int(got["reason"][r]), kept=int(got["kept"][r]),
                mean_var=pu.words32(got["mean_var"][r]), A=pu.words32(got["A"][r]).ravel(), pi=pu.words32(got["pi"][r]))


def same_member(a, b, what=None):
    for key in ("trace", "mean_var", "A", "pi"):
        assert np.array_equal(np.asarray(a[key]).ravel(), np.asarray(b[key]).ravel()), (what, key)
    assert (a["steps"], a["reason"], a["kept"]) == (b["steps"], b["reason"], b["kept"]), what


def twin(g, starts, r, max_steps, rel_tol, use_prior):
    """member r as the definition has it, on the same chain"""
    g.set_parameters(starts[0][r], starts[1][r], starts[2][r])
    trace, steps, reason, kept = g.em_fit(max_steps, rel_tol=rel_tol, use_prior=use_prior)
    A, pi = g.transitions()
    return dict(trace=pu.words(trace), steps=steps, reason=reason, kept=kept, mean_var=pu.words32(g.theta()), A=pu.words32(A).ravel(), pi=pu.words32(pi))


def check_batch(g, starts, program=None, ref=(), max_steps=5, rel_tol=0.0, use_prior=False, self_trans=True, what=None):
    """the batch (which only reads the chain) against the twin of every member and the restatement of the members `ref`"""
    before = parameters(g)
    R = len(starts[0])
    got = g.em_fit_many(starts=starts, max_steps=max_steps, rel_tol=rel_tol, use_prior=use_prior, install=False)
    assert parameters(g) == before, what
    assert g.em_many_info()["members"] == R
    case = pu.chain_case(g, self_trans)
    for r in range(R):
        m = member_words(got, r)
        assert np.isnan(got["trace"][r, m["steps"] + 1:]).all(), (what, r)      # (an entry before that may be one too: a fit's own)
        assert pu.words([got["objective"][r]])[0] == m["trace"][-1], (what, r)
        same_member(m, twin(g, starts, r, max_steps, rel_tol, use_prior), (what, r, "twin"))
        if r in ref:
            want = eu.run_program(program, "fit", dict(case, mean_var=starts[0][r], A=starts[1][r], pi=starts[2][r]), use_prior=use_prior, prior=prior(g),
                                  max_steps=max_steps, rel_tol=rel_tol)
            same_member(m, want, (what, r, "restatement"))
    assert got["best"] == mu.best(got["reason"].tolist(), got["objective"].tolist()), what
    g.set_parameters(np.frombuffer(before[0], f32), np.frombuffer(before[1], f32), np.frombuffer(before[2], f32))
    return got


# ---------------------------------------------------------------------------------------------- shapes
@pytest.mark.parametrize("T", [2, 3, 65])
def test_tiny_traces(hml, program, T):
    g = chain(hml, ol.trace(1000, 3, 2)[:T].copy(), 2, seed=12, sweeps=10)
    check_batch(g, g.em_starts(3, 4), program, ref=(0, 2), what=T)


def test_one_block(hml, program):
    g = hml.Chain(device=0, seed=12)
    g.load(np.array([0.3], np.float32))
    g.em_nig4 = np.array([2.0, 1.0, 0.0, 1.0], np.float32)
    g.set_model(2, g.em_nig4)
    g.sample_prior()
    g.create_blocks(1.0)
    assert g.num_blocks() == 1
    check_batch(g, g.em_starts(2, 1), program, ref=(0, 1), max_steps=2, use_prior=True, what="B = 1")


@pytest.mark.parametrize("B,R", [(64, 3), (65, 3), (66, 2), (4097, 3), (70000, 2)])
def test_every_position_a_block(hml, program, B, R):
    g = chain(hml, ol.trace(B, 5, 4), 5, every_position=True)
    assert g.num_blocks() == B
    check_batch(g, g.em_starts(R, 7), program, ref=(1,), what=B)


@pytest.mark.parametrize("K,R", [(2, 3), (8, 3), (9, 3), (16, 3), (17, 3), (64, 2)])
def test_numbers_of_states(hml, program, K, R):
    B = 4100 if K <= 16 else 1300        # (two levels of the trees either way; the restatement at 64 states takes its time)
    g = chain(hml, ol.trace(B, min(K, 5), 7), K, every_position=True)
    assert g.num_blocks() == B
    check_batch(g, g.em_starts(R, 11), program, ref=(R - 1,), what=K)


@pytest.mark.parametrize("prior_on", [False, True])
def test_seventeen_members_over_blocks_of_many_positions(hml, program, prior_on):
    g = chain(hml, ol.trace(30000, 5, 8), 5)
    assert g.num_blocks() < 30000
    got = check_batch(g, g.em_starts(17, 3), program, ref=(0, 16), use_prior=prior_on, what=prior_on)
    assert len({got["mean_var"][r].tobytes() for r in range(17)}) > 1


def test_two_dimensions_two_parameters(hml, program):
    T = 4096
    x = np.stack([ol.trace(T, 3, 1), ol.trace(T, 3, 2)], axis=1).reshape(-1)
    g = chain(hml, x, 4, dims=(2, 2), every_position=True)
    starts = g.em_starts(3, 5)
    assert starts[0].shape == (3, 4)
    check_batch(g, starts, program, ref=(2,), what="D = 2")


@pytest.mark.parametrize("name", hi.family("ties")[:1])
def test_integer_data_full_of_ties(hml, program, name):
    fn, K, _ = hi.INPUTS[name]
    g = chain(hml, hi.data(name)[:20000], K, seed=hi.SEED[name], sweeps=5)
    check_batch(g, g.em_starts(3, 2), program, ref=(1,), what=name)


def test_self_transitions_off(hml, program):
    g = chain(hml, ol.trace(20000, 3, 5), 3, self_trans=False)
    check_batch(g, g.em_starts(3, 6), program, ref=(2,), self_trans=False)


def test_compat_context(hml, program):
    g = chain(hml, ol.trace(20000, 3, 6), 3, options=[("compat", 1)], sweeps=5)
    g.create_blocks(g.threshold())
    check_batch(g, g.em_starts(2, 8), program, ref=(1,), use_prior=True, what="compat")


def test_starts_are_the_header_s(hml):
    g = chain(hml, ol.trace(20000, 3, 5), 3)
    mv, (A, pi) = g.theta(), g.transitions()
    for seed, spread in ((1, 1.0), (0xFEDCBA9876543210, 0.3)):
        got = g.em_starts(17, seed, spread)
        want = mu.starts(3, 3, 17, seed, spread, mv, A, pi)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want))
    for spread in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(hml.HmlError):
            g.em_starts(3, 1, spread)


# ---------------------------------------------------------------------------------------------- the cut, the company
def test_the_cut_is_invisible(hml):
    """the same batch in groups of one, of two and in one group: the same words; launch sets are counted per group and E-step"""
    R = 5
    g = chain(hml, ol.trace(20000, 5, 4), 5, every_position=True)
    starts = g.em_starts(R, 9)
    estimate = 2 * g.num_blocks() * 5 * 8            # alpha and beta: the greater part of a member's bytes
    budgets = {1: 1}
    for mult in np.arange(2.0, 6.01, 0.25):          # (a budget that holds two members and not three, found by asking)
        g.set_em_batch_bytes(int(mult * estimate))
        g.em_fit_many(starts=starts, max_steps=0, install=False)
        if g.em_many_info()["group_size"] == 2:
            budgets[2] = int(mult * estimate)
            break
    assert 2 in budgets
    budgets[R] = 0
    results = {}
    for G, n_bytes in budgets.items():
        g.set_em_batch_bytes(n_bytes)
        results[G] = g.em_fit_many(starts=starts, max_steps=5, rel_tol=-1.0, install=False)       # (all members run all steps)
        info = g.em_many_info()
        assert info["group_size"] == G and info["groups"] == -(-R // G) and info["esteps"] == 6, (G, info)
        assert info["launch_sets"] == info["groups"] * info["esteps"], (G, info)
    for G in (1, 2):
        for key, v in results[R].items():
            assert np.asarray(v).tobytes() == np.asarray(results[G][key]).tobytes(), (G, key)
    # ... and the company: member r alone
    for r in (0, 3):
        alone = g.em_fit_many(starts=tuple(s[r:r + 1] for s in starts), max_steps=5, rel_tol=-1.0, install=False)
        same_member(member_words(alone, 0), member_words(results[R], r), ("alone", r))
        assert alone["best"] == 0


# ---------------------------------------------------------------------------------------------- ragged stops
@pytest.mark.parametrize("name", sorted(mu.RAGGED_CASES))
def test_ragged_stops(hml, tmp_path, name):
    """the traces and starts of the fixtures of tests/test_em_many_cpu.py, every position a block (a chain forms its own blocks:
    the fixtures' 300 cannot be given to it), at their tolerance and 30 steps: members leave the batch at different steps, and the
    words of every member, the winner and the installed floats are the restatement's, fed the chain's blocks"""
    f = mu.RAGGED_CASES[name]
    many = mu.build_programs(tmp_path, sanitized=False)["plain"]
    g = chain(hml, mu.switching_trace(f["trace_seed"]), f["K"], self_trans=f["self_trans"], every_position=True)
    fixture = mu.ragged_case(name)
    g.set_parameters(fixture[0]["mean_var"], fixture[0]["A"], fixture[0]["pi"])
    starts = g.em_starts(f["R"], f["seed"])
    case = pu.chain_case(g, f["self_trans"])
    want, win = mu.program_fits(many, case, *starts, **mu.RAGGED)
    if name == "k3":            # (with every position a block the four-state members all run the 30 steps; the three-state ones do not)
        assert len({m["steps"] for m in want}) > 1
    else:
        assert win >= 1 and mu.objective_of(want[win]) > mu.objective_of(want[0])
    got = g.em_fit_many(starts=starts, install=True, **mu.RAGGED)
    for r in range(f["R"]):
        m = member_words(got, r)
        same_member(m, want[r], (name, r))
        assert np.isnan(got["trace"][r, m["steps"] + 1:]).all()
    assert got["best"] == win and win >= 0
    assert g.em_many_info()["esteps"] == max(m["steps"] for m in want) + 1
    assert np.array_equal(pu.words32(g.theta()), want[win]["mean_var"])
    A, pi = g.transitions()
    assert np.array_equal(pu.words32(A).ravel(), want[win]["A"]) and np.array_equal(pu.words32(pi), want[win]["pi"])
    # installed as a single fit from that start leaves it: the twin's whole model
    h = chain(hml, mu.switching_trace(f["trace_seed"]), f["K"], self_trans=f["self_trans"], every_position=True)
    twin(h, starts, win, mu.RAGGED["max_steps"], mu.RAGGED["rel_tol"], False)
    assert parameters(h) == parameters(g) and h.threshold() == g.threshold()


# ---------------------------------------------------------------------------------------------- a degenerate member
def unreachable(hml):
    """tests/test_gpu_em.py's block no path reaches: (chain, the degenerate start)"""
    x = np.random.default_rng(2).normal(0, 0.3, 300).astype(np.float32)
    x[1:3] += 40.0
    g = chain(hml, x, 3, sweeps=1, every_position=True, self_trans=False)
    A = np.array([[0.5, 0.25, 0.25], [1.0, 0.0, 0.0], [0.25, 0.25, 0.5]], np.float32)
    return g, (np.array([0.0, 1.0, 0.0, 1.0, 40.0, 1.0], np.float32), A, np.array([0.0, 1.0, 0.0], np.float32))


def test_a_degenerate_member(hml, program):
    g, bad = unreachable(hml)
    good = g.em_starts(2, 3)
    starts = tuple(np.stack([good[i][0], bad[i], good[i][1]]) for i in range(3))
    got = check_batch(g, starts, program, ref=(1, 2), self_trans=False)
    assert (got["steps"][1], got["reason"][1], got["kept"][1]) == (0, hml.EM_DEGENERATE, 0) and got["objective"][1] == -np.inf
    assert got["steps"][0] >= 1 and got["steps"][2] >= 1 and got["best"] in (0, 2)
    assert got["mean_var"][1].tobytes() == bad[0].tobytes()


def test_a_batch_without_a_candidate(hml):
    g, bad = unreachable(hml)
    before = parameters(g)
    got = g.em_fit_many(starts=tuple(np.stack([v, v]) for v in bad), max_steps=5, install=True)
    assert got["best"] == -1 and got["reason"].tolist() == [hml.EM_DEGENERATE] * 2 and got["steps"].tolist() == [0, 0]
    assert parameters(g) == before


# ---------------------------------------------------------------------------------------------- repair per member
def test_repair_per_member(hml):
    """tests/test_gpu_posterior.py's weakly separated trace at W = 64: one member at the weakly separated parameters, one at
    well-separated ones"""
    from tests.test_gpu_posterior import weak_chain
    g = weak_chain(hml)
    weak = (g.theta(),) + tuple(g.transitions())
    well = (np.stack([2.0 * np.arange(5) - 2.0, np.full(5, 0.25)], 1).ravel().astype(f32), weak[1], weak[2])
    starts = tuple(np.stack([a, b]) for a, b in zip(weak, well))
    g.set_option("posterior_W", 64)
    alone = g.em_fit_many(starts=tuple(s[1:] for s in starts), max_steps=2, rel_tol=-1.0, install=False)
    seen = {}
    for rounds in (8, 0):
        g.set_option("posterior_rounds", rounds)
        got = check_batch(g, starts, max_steps=2, rel_tol=-1.0, what=rounds)
        seen[rounds] = g.em_many_info()
        same_member(member_words(got, 1), member_words(alone, 0), ("the well-separated member", rounds))
    assert seen[8]["stale_fwd"] > 0 and seen[8]["stale_bwd"] > 0 and seen[8]["rounds"] >= 1, seen
    assert seen[0]["rounds"] == 0 and seen[0]["serial_chunks"] > 0, seen


# ---------------------------------------------------------------------------------------------- refusals, memory, side effects
def test_a_refused_start(hml):
    g = chain(hml, ol.trace(5000, 3, 3), 3)
    starts = g.em_starts(4, 1)
    starts[0][2, 3] = 0.0
    before = parameters(g)
    with pytest.raises(hml.HmlError) as e:
        g.em_fit_many(starts=starts, max_steps=2)
    assert "must be positive" in str(e.value) and "(start 2)" in str(e.value)
    starts[0][2, 3] = np.nan
    with pytest.raises(hml.HmlError) as e:
        g.em_fit_many(starts=starts, max_steps=2)
    assert "finite" in str(e.value) and "(start 2)" in str(e.value)
    assert parameters(g) == before
    with pytest.raises(hml.HmlError):
        g.em_fit_many(starts=tuple(np.zeros((0,) + s.shape[1:], f32) for s in starts))
    fresh = hml.Chain(device=0, seed=1)
    fresh.load(ol.trace(100, 3, 3))
    fresh.set_model(3, fresh.autoprior(0.2, 0.9))
    fresh.sample_prior()
    with pytest.raises(hml.HmlError) as e:
        fresh.em_fit_many(starts=starts, max_steps=1)
    assert "no blocks yet" in str(e.value)


def test_the_call_keeps_no_device_memory_and_survives_failed_allocations(hml):
    g = chain(hml, ol.trace(5000, 3, 3), 3, every_position=True)
    g.set_option("posterior_W", 1)      # (stale chunks: the repair kernels run too)
    starts = g.em_starts(3, 2)
    gc.collect()      # (chains that earlier tests dropped without closing go first: the totals below are this test's alone)
    before, params = hml.device_memory_live(), parameters(g)
    flat = lambda r: [np.asarray(v).tobytes() for v in r.values()]
    call = lambda: g.em_fit_many(starts=starts, max_steps=1, install=False)
    hml.debug_fail_allocation(10 ** 9)
    good = call()
    n_alloc = hml.debug_fail_allocation(0)
    assert n_alloc >= 20 and hml.device_memory_live() == before
    for n in range(1, n_alloc + 1):
        hml.debug_fail_allocation(n)
        with pytest.raises(hml.HmlError) as e:
            call()
        hml.debug_fail_allocation(0)
        assert e.value.code == 2 and "out of memory" in str(e.value), n
        assert hml.device_memory_live() == before and parameters(g) == params, n
        if n % 8 == 0:
            assert flat(call()) == flat(good), n          # the next call succeeds
    assert flat(call()) == flat(good) and hml.device_memory_live() == before


def test_a_batch_that_is_not_installed_only_reads(hml):
    x = ol.trace(40000, 3, 13)

    def run(batch):
        g = chain(hml, x, 3, seed=5, sweeps=0)
        g.iterate("F", 6, 2)
        if batch:
            got = g.em_fit_many(n_starts=4, seed=3, max_steps=3, install=False)
            assert got["best"] >= 0
        g.iterate("F", 5, 1)
        g.iterate("M", 2, 1)
        g.sync()
        seg, cnt = g.marginals_rle()
        return g.states(), g.theta(), g.transitions(), seg, cnt, g.blocks()

    a, b = run(False), run(True)
    flat = lambda r: [np.asarray(v).tobytes() for part in r for v in (part if isinstance(part, tuple) else (part,))]
    assert flat(a) == flat(b)


def test_the_winner_is_installed(hml):
    g = chain(hml, ol.trace(20000, 3, 21), 3)
    starts = g.em_starts(4, 5)
    got = g.em_fit_many(starts=starts, max_steps=5)
    win = got["best"]
    assert win >= 0 and got["objective"][win] == np.nanmax(got["objective"])
    assert parameters(g) == [got["mean_var"][win].tobytes(), got["A"][win].tobytes(), got["pi"][win].tobytes()]
    assert pu.words([g.posterior()[1]])[0] == pu.words([got["objective"][win]])[0]     # log p(y | theta-hat) of the installed parameters
    g.iterate("F", 3, 0)                          # the chain's next sweeps run
    g.sync()
    assert np.isfinite(g.theta()).all()

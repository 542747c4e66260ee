"""The differential tests once more under the test mode of the owner of device memory (hml_debug_guard_allocations, DESIGN.md
section 3f): a guard band of 4096 bytes on both sides of every allocation of the library and a body of 0xFF bytes.  A store past
either end of an array damages a band, and the fixture's check names the allocation; memory that a kernel reads before anybody
wrote it is NaN, -1 or the largest integer instead of the zeros a fresh process finds there, and the comparison with the checker
(or with the restatements) fails.  Every test asserts what the test of its path asserts - bit for bit - and the clean guard
report on top.  The shapes are the ones where the arrays are full to their last element: every position a block, so that B = T
is the capacity of the per-block arrays, at lengths around every unit the kernels work in.

Wall time of the module on one MI355X, measured once: 58 s for its 355 tests; the slowest - 25 batches of chains - 5.8 s."""
import gc
import os

import numpy as np
import pytest
import torch  # noqa: F401  (the caller-given device buffers; imported at collection, not inside the first test)

from tests import guarded_util as gu
from tests import oracle_lib as ol
from tests import posterior_util as pu
from tests.fuzz_util import fuzz
from tests.readout_fuzz_util import fuzz_readouts
from tests.test_gpu_forward_loads import SCHEME, check, set_up
from tests.test_gpu_parity import compare_state, make_pair, run_both, setup_model
from tests.words_util import DEVICE_NAN, HOST_NAN, same_words  # noqa: F401

pytestmark = pytest.mark.gpu

MIXTURE_SCHEME = [("F", 2, 0), ("M", 2, 1), ("F", 1, 1)]   # a mixture sweep between forward-backward sweeps, two recorded


@pytest.fixture
def guarded(hml):
    """arms the mode (4096 bytes, poison), and afterwards - whatever the test did - checks every guard and disarms"""
    earlier = hml.debug_check_guards(reset=True)      # (a guarded buffer freed since the last teardown - a chain collected late)
    assert earlier == {"damaged": 0}, earlier
    hml.debug_guard_allocations(gu.GUARD_BYTES, poison=True)
    try:
        yield hml
    finally:
        try:
            report = hml.debug_check_guards(reset=True)
        finally:
            hml.debug_guard_allocations(0)
    assert report == {"damaged": 0}, report


def clean(hml):
    """the check in mid-test, while the chains are alive: their guards are read back"""
    report = hml.debug_check_guards(reset=False)
    assert report == {"damaged": 0}, report


# ------------------------------------------------------------------------------------------------------------ a. self-test
def test_the_mode_detects(hml):
    """hml_debug_guard_selftest: the poisoned body reads back as 0xFF; a byte set behind the body is found by the check, a byte
    set before it by the buffer's free - from the host, in memory the library owns.  It leaves the mode off and the report
    empty, and with the mode off a chain's allocations are not registered."""
    hml.debug_check_guards(reset=True)
    gc.collect()      # (chains that earlier tests dropped without closing go first)
    before = hml.device_memory_live()
    hml.debug_guard_selftest()
    assert hml.debug_check_guards(reset=False) == {"damaged": 0}
    assert hml.device_memory_live() == before


def test_the_live_totals_count_the_callers_bytes(guarded):
    """hml_device_memory_live under the mode: the bytes the owners asked for, without the guards"""
    hml = guarded
    x = ol.trace(1000, 3, 1)
    gc.collect()      # (chains that earlier tests dropped without closing go first)

    def held():
        before = hml.device_memory_live()
        g = hml.Chain(device=0, seed=3)
        g.load(x)
        g.set_model(3, g.autoprior())
        now = hml.device_memory_live()
        g.close()
        assert hml.device_memory_live() == before
        return now[0] - before[0], now[1] - before[1]

    with_guards = held()
    hml.debug_guard_allocations(0)
    without = held()
    hml.debug_guard_allocations(gu.GUARD_BYTES, poison=True)
    assert with_guards == without and with_guards[1] > 0


# ------------------------------------------------------------------------------------------- b. full-capacity sweeps
def full_chain(hml, T, K, scheme=SCHEME, compat=False, dims=None):
    """checker and chain of a trace whose every position is a block, after the scheme: (o, g).  compat: the reference-compatible
    mode against the checker's reference mode; dims = (D, P): D data dimensions over P parameters a dimension, K = P ** D."""
    if compat or dims:
        D, P = dims or (1, None)
        levels = P if dims else (K if K in ol.LEVELS else 6)
        x = np.stack([ol.trace(max(T, 2), levels, 7 + d)[:T] for d in range(D)], axis=1).reshape(-1)
        mode = dict(rng=ol.RNG_MT, math=ol.MATH_LIBM, reduce=ol.REDUCE_REF) if compat else dict(rng=ol.RNG_CTR, math=ol.MATH_DEV, reduce=ol.REDUCE_DEV)
        o = ol.OracleChain(K=K, seed=42, chain=0, weight_mult=1e9, **mode)
        g = hml.Chain(device=0, seed=42, chain_id=0)
        if compat:
            g.set_option("compat", 1)
        if dims:
            o.set_dimensions(D, P)
            g.set_dimensions(D, P)
        o.load(x)
        g.load(x)
        g.scale_weights(1e9)
    else:
        x, o, g = make_pair(hml, T, K, 7, 42, weight_mult=1e9)
    set_up(o, g, x, K)
    g._pending_prior = True
    o.set_record(marginals=True)
    run_both(o, g, scheme)
    return o, g


def full_case(hml, T, K, what, **kw):
    o, g = full_chain(hml, T, K, **kw)
    check(hml, o, g, T, "%s, T = %d, %d states" % (what, T, K))     # every position a block; blocks, states, theta, A, pi; marginals
    clean(hml)
    g.close()
    o.close()


DEFAULT_CASES = gu.spread(gu.LENGTHS, gu.DEFAULT_K)
MID_CASES = gu.spread(gu.LENGTHS, gu.MID_K)
WEAK_CASES = gu.spread(gu.WEAK_LENGTHS, gu.WEAK_K)
WIDE_CASES = gu.spread(gu.LENGTHS, gu.WIDE_K)
COMPAT_CASES = gu.spread(gu.LENGTHS, gu.COMPAT_K)


@pytest.mark.parametrize("T,K", DEFAULT_CASES)
def test_full_capacity_default_path(guarded, T, K):
    full_case(guarded, T, K, "default path")


@pytest.mark.parametrize("T,K", MID_CASES)
def test_full_capacity_chunks_of_eight(guarded, monkeypatch, T, K):
    monkeypatch.setenv("HML_MID_MIN_BLOCKS", "1")
    full_case(guarded, T, K, "chunks of 8")


@pytest.mark.parametrize("L", [32, 1024])
@pytest.mark.parametrize("T,K", WEAK_CASES)
def test_full_capacity_weakly_compressed(guarded, monkeypatch, T, K, L):
    monkeypatch.setenv("HML_DENSE_MIN_BLOCKS", "500")
    monkeypatch.setenv("HML_TRELLIS_L", str(L))
    full_case(guarded, T, K, "weakly compressed geometry, chunks of %d" % L)


@pytest.mark.parametrize("T,K", WIDE_CASES)
def test_full_capacity_many_states(guarded, monkeypatch, T, K):
    """chunks of the default length, of 1 block and of 64: in turn over the cases, all three at the lengths where every K runs"""
    i = WIDE_CASES.index((T, K))
    for L in ([None, 1, 64] if T in gu.EVERY_K_AT else [[None, 1, 64][i % 3]]):
        if L is None:
            monkeypatch.delenv("HML_WIDE_L", raising=False)
        else:
            monkeypatch.setenv("HML_WIDE_L", str(L))
        full_case(guarded, T, K, "many states, HML_WIDE_L = %s" % L)


@pytest.mark.parametrize("T,K", [(1, 17), (64, 20), (65, 64), (1025, 20), (4097, 17)])
def test_full_capacity_many_states_a_state_a_lane(guarded, monkeypatch, T, K):
    monkeypatch.setenv("HML_WIDE_LANES", "0")
    full_case(guarded, T, K, "many states, a state a lane")


@pytest.mark.parametrize("T,K", COMPAT_CASES)
def test_full_capacity_compat(guarded, monkeypatch, T, K):
    """the sequential form and 60 chunks: in turn over the cases, both at the lengths where every K runs"""
    i = COMPAT_CASES.index((T, K))
    for chunks in ([1, 60] if T in gu.EVERY_K_AT else [[1, 60][(i + i // 2) % 2]]):
        monkeypatch.setenv("HML_COMPAT_CHUNKS", str(chunks))
        full_case(guarded, T, K, "compat, %d chunks" % chunks, compat=True)


@pytest.mark.parametrize("P", [2, 3])
@pytest.mark.parametrize("T", gu.LENGTHS)
def test_full_capacity_two_dimensions(guarded, T, P):
    full_case(guarded, T, P * P, "C 2 %d" % P, dims=(2, P))


def attached_case(hml, monkeypatch, T, split, scheme):
    """three chains on one construction through hml_iterate_many, the block structure by the fused many-chain kernel (0) and in two
    launches (1); 3 states under the one, 5 under the other"""
    monkeypatch.setenv("HML_FM_SPLIT", str(split))
    K = gu.MANY_K[split]
    x = ol.trace(max(T, 2), K, 7)[:T]
    pairs = []
    for chain in range(3):
        o = ol.OracleChain(K=K, seed=9, chain=chain, rng=ol.RNG_CTR, math=ol.MATH_DEV, reduce=ol.REDUCE_DEV, weight_mult=1e9)
        o.load(x)
        g = hml.Chain(device=0, seed=9, chain_id=chain)
        if chain == 0:
            g.load(x)
            g.scale_weights(1e9)   # (before the others attach: shared weights are not rescaled)
        else:
            g.attach(pairs[0][1])
        set_up(o, g, x, K)
        o.token("F")
        g.sample_prior()
        o.set_record(marginals=True)
        pairs.append((o, g))
    gs = [g for _, g in pairs]
    for m, n, t in scheme:
        for o, _ in pairs:
            o.iterate(m, n, t)
        hml.iterate_many(gs, m, n, t)
    for chain, (o, g) in enumerate(pairs):
        g.sync()
        check(hml, o, g, T, "attached chain %d of 3, T = %d, split %d" % (chain, T, split))
    clean(hml)
    for o, g in reversed(pairs):
        g.close()
        o.close()


@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("T", gu.LENGTHS)
def test_full_capacity_three_attached_chains(guarded, monkeypatch, T, split):
    attached_case(guarded, monkeypatch, T, split, SCHEME)


@pytest.mark.parametrize("T,split", [(65, 0), (1025, 1)])
def test_full_capacity_three_attached_chains_mixture_sweeps(guarded, monkeypatch, T, split):
    attached_case(guarded, monkeypatch, T, split, MIXTURE_SCHEME)


@pytest.mark.parametrize("T", gu.GROWTH_LENGTHS)
@pytest.mark.parametrize("path,K", [("default", 2), ("default", 5), ("default", 16), ("wide", 20), ("compat", 3)])
def test_full_capacity_after_a_growth(guarded, monkeypatch, path, K, T):
    """HML_MAX_BLOCKS = 64: per-block arrays of exactly the 64 blocks the trace has, of one less than it has, and grown several
    times - the arrays a growth hands out are recycled memory.  (Univariate models: with several data dimensions the capacity is
    T from the start.)"""
    monkeypatch.setenv("HML_MAX_BLOCKS", "64")
    scheme = MIXTURE_SCHEME if (T, K) in ((1025, 5), (65, 20)) else SCHEME      # (a mixture sweep on the default and the many-state path)
    o, g = full_chain(guarded, T, K, scheme=scheme, compat=path == "compat")
    check(guarded, o, g, T, "%s after a growth, T = %d, %d states" % (path, T, K))
    st = g.stats()
    assert (st["buffer_growths"] >= 1 and st["block_capacity"] > 64) if T > 64 else st["block_capacity"] >= 64, st
    clean(guarded)
    g.close()
    o.close()


@pytest.mark.parametrize("path,T,K", [("default", 65, 5), ("default", 1025, 8), ("mid", 1025, 5), ("weak", 1025, 5), ("wide", 65, 20), ("wide", 1025, 17),
                                      ("compat", 1025, 3), ("C 2 2", 257, 4)])
def test_full_capacity_mixture_sweeps(guarded, monkeypatch, path, T, K):
    if path == "mid":
        monkeypatch.setenv("HML_MID_MIN_BLOCKS", "1")
    if path == "weak":
        monkeypatch.setenv("HML_DENSE_MIN_BLOCKS", "500")
    full_case(guarded, T, K, "%s with a mixture sweep" % path, scheme=MIXTURE_SCHEME, compat=path == "compat", dims=(2, 2) if path == "C 2 2" else None)


# ------------------------------------------------------------------------------------------------ c. fuzz slices
def _slice(hml, name):
    n, seed, mode = gu.FUZZ_SLICES[name]
    lines = []
    assert fuzz(hml, n, seed, log=lines.append, **mode) == n
    assert len(lines) == n
    return lines


@pytest.mark.parametrize("name", ["plain", "compat", "wide"])
def test_fuzz_slice(guarded, name):
    """the slice is the one tests/test_guarded_memory_cpu.py walked - line for line - and not hollow"""
    lines = _slice(guarded, name)
    n, seed, mode = gu.FUZZ_SLICES[name]
    for line, c in zip(lines, gu.walk(n, seed, **mode)):
        if "both raise" not in line:
            assert all(part in line for part in gu.line_of(c)), (line, c)
    assert not gu.wanting(lines), gu.wanting(lines)


def test_fuzz_slice_with_a_tiny_block_capacity(guarded, monkeypatch):
    monkeypatch.setenv("HML_MAX_BLOCKS", "64")
    _slice(guarded, "max_blocks_64")


def test_fuzz_slice_of_batched_chains(guarded):
    _slice(guarded, "many")


@pytest.mark.parametrize("part", range(len(gu.FUZZ_HOSTILE)))
def test_fuzz_slice_on_hostile_inputs(guarded, part):
    n, seed, mode = gu.FUZZ_HOSTILE[part]
    assert fuzz(guarded, n, seed, data="hostile", **mode) == n


@pytest.mark.parametrize("name", list(gu.READOUT_SLICES))
def test_readout_fuzz_slice(guarded, name):
    n, seed, mode = gu.READOUT_SLICES[name]
    assert fuzz_readouts(guarded, n, seed, **mode) == n


# ------------------------------------------------------------------------------------------------ f. text reader
def same(a, b):
    return a.size == b.size and np.array_equal(a.view(np.uint32), b.view(np.uint32))


SMALLEST_CHUNK = 256     # hml_text_open takes 256 bytes to 256 MiB


def parsed(hml, text, chunk):
    want, stopped = ol.parse_text(text)
    got, info = hml.parse_text(text, chunk_bytes=chunk, with_info=True)
    assert same(got, want) and info["stopped"] == stopped and info["bytes"] == len(text), (len(text), chunk, got.size, want.size)
    return want, info


@pytest.mark.parametrize("chunk", [SMALLEST_CHUNK, 65536])
@pytest.mark.parametrize("size", [4096, 8192, 4096 * 3 + 1, 65536, 65537])
def test_text_of_as_many_tokens_as_a_tile_and_a_chunk_hold(guarded, size, chunk):
    """"1 " over and over: a token every second byte, which is what the values' array is sized for (chunk_bytes / 2 + 1) - to
    exactly one tile of 4096 bytes, two, three and a byte, and a chunk of 65536 and a byte"""
    text = (b"1 " * (size // 2 + 1))[:size]
    want, _ = parsed(guarded, text, chunk)
    assert want.size == (size + 1) // 2


@pytest.mark.parametrize("n", [65536, 65537])
def test_text_of_as_many_irregular_tokens_as_the_list_holds(guarded, n):
    """21-digit tokens, which the device hands to the host: exactly the list's 65536 entries, and one more - then the chunk goes
    through the stream extraction whole"""
    text = (" ".join("1.%020d" % (i * 7919) for i in range(n)) + "\n").encode()
    _, info = parsed(guarded, text, 0)
    assert (info["host_chunks"], info["irregular_tokens"]) == ((0, n) if n == 65536 else (1, 0)), info


@pytest.mark.parametrize("chunk", [SMALLEST_CHUNK, 65536])
def test_text_that_ends_on_a_tile_and_without_a_newline(guarded, chunk):
    """a token whose last byte is the tile's last, one that straddles two tiles, and texts that end without a newline - on the last
    byte of a tile, and a byte into the next"""
    texts = {
        4096: b"2.5 " * 1022 + b"1.25 -17",                   # the last token ends on the tile's last byte, no newline
        4097: b"2.5 " * 1023 + b"-1.25",                      # a token that straddles two tiles, no newline
        4098: b"2.5 " * 1023 + b"1.5\n" + b"77",              # a newline on the tile's last byte, the last token in the next tile
        4101: b"2.5 " * 1022 + b"1.25 -17" + b" 3.5\n",       # ... ends on the tile's last byte, and the text goes on
    }
    counts = {4096: (1024, -17.0), 4097: (1024, -1.25), 4098: (1025, 77.0), 4101: (1025, 3.5)}
    for size, text in texts.items():
        assert len(text) == size
        want, _ = parsed(guarded, text, chunk)
        assert (want.size, float(want[-1])) == counts[size]


# ------------------------------------------------------------------------------------------------ g. pooling in one process
def pooled_chain(hml, x, K, chain):
    o = ol.OracleChain(K=K, seed=21, chain=chain, rng=ol.RNG_CTR, math=ol.MATH_DEV, reduce=ol.REDUCE_DEV, weight_mult=1e9)
    g = hml.Chain(device=0, seed=21, chain_id=chain)
    o.load(x)
    g.load(x)
    g.scale_weights(1e9)
    setup_model(o, g, K)
    o.token("F")
    g.sample_prior()
    o.set_record(marginals=True)
    o.iterate("F", 6, 2)
    g.iterate("F", 6, 2)
    g.sync()
    return o, g


def pooled_marginals(os_, K, T):
    """what pooling leaves in every chain: the checker's dense marginals under the common labels, summed, as segments"""
    from hammlet_amd import chains
    dense, bnd, perms = np.zeros((K, T), np.int64), np.zeros(T, np.int64), []
    for o in os_:
        lens = [int(l.split("\t")[0]) for l in o.text("marginals").strip().split("\n")]
        bnd[np.cumsum([0] + lens[:-1])] += 1
        perms.append(chains.relabel_permutation(o.theta()[0::2].copy()))
        dense += o.marginals_dense()[perms[-1]]
    starts = np.flatnonzero(bnd)
    cols = int(np.flatnonzero(dense.any(axis=1)).max()) + 1
    return np.diff(np.append(starts, T)), dense[:cols, starts].T, perms


@pytest.mark.parametrize("K", [2, 16])
@pytest.mark.parametrize("T", [17, 1025])
def test_pooling_entry_points_of_one_process(guarded, T, K):
    """hml_allreduce_marginals_perm over three chains of one device (acc and tmp), the export / install pair with the sum done by the
    caller into a payload of exactly hml_pool_payload_size elements, and hml_pool_marginals with a one-rank communicator in both
    forms (the payload and the handshake buffer) - each against the checker's chains"""
    hml = guarded
    x = ol.trace(T, K if K in ol.LEVELS else 6, 3)
    made = [pooled_chain(hml, x, K, c) for c in range(3)]
    os_, gs = [o for o, _ in made], [g for _, g in made]
    for o, g in made:
        compare_state(o, g)
    seg_e, cnt_e, perms_e = pooled_marginals(os_, K, T)
    # export, external sum, install: into a fourth chain's twin of chain 0
    n = gs[0].pool_payload_size()
    assert n == (K + 1) * (T + 1) + 1 + K
    margin = 1024
    bufs = [torch.full((n + 2 * margin,), -7, dtype=torch.int32, device="cuda") for _ in range(3)]
    for g, b in zip(gs, bufs):
        g.pool_export(b[margin:margin + n].data_ptr())
    torch.cuda.synchronize()
    for b in bufs:
        assert bool((b[:margin] == -7).all()) and bool((b[margin + n:] == -7).all())
    total = bufs[0][margin:margin + n] + bufs[1][margin:margin + n] + bufs[2][margin:margin + n]
    torch.cuda.synchronize()
    o4, twin = pooled_chain(hml, x, K, 0)
    twin.pool_install(total.data_ptr())
    seg, cnt = twin.marginals_rle()
    assert np.array_equal(seg, seg_e) and np.array_equal(cnt, cnt_e)
    # one rank through the communicator, dense payload and boundary lists
    for form in (1, 2):
        o5, g5 = pooled_chain(hml, x, K, 1)
        pool = hml.Pool(0, 0, 1, hml.Pool.unique_id())
        pool.set_form(form)
        perm = pool.marginals(g5)
        assert np.array_equal(perm, perms_e[1])
        s1, c1, _ = pooled_marginals([os_[1]], K, T)
        seg, cnt = g5.marginals_rle()
        assert np.array_equal(seg, s1) and np.array_equal(cnt, c1), form
        clean(hml)
        pool.close()
        g5.close()
        o5.close()
    # three chains summed on their device
    perms = hml.allreduce_marginals(gs, with_perms=True)
    for i, g in enumerate(gs):
        assert np.array_equal(perms[i], perms_e[i])
        seg, cnt = g.marginals_rle()
        assert np.array_equal(seg, seg_e) and np.array_equal(cnt, cnt_e)
        assert g.recorded_sweeps() == 3 * 3
    clean(hml)
    for o, g in made + [(o4, twin)]:
        g.close()
        o.close()


# ------------------------------------------------------------------------------------------------ d. exact inference
# (hml_infer.hip: the scratch of a call is freed inside it, so its guards are checked by the free alone)
EXACT_LENGTHS = [1, 2, 3, 4, 5, 63, 64, 65, 1025]
GEOMETRIES = [(L, W, rounds) for L in (4, 64) for W in (1, 4) for rounds in (0, 8)]


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    """the restatements for one host thread of the decode, the smoothing, the E-step / fit and the pairwise read-outs"""
    from tests import em_util, pairs_util, posterior_util, viterbi_util
    return {name: util.build_programs(tmp_path_factory.mktemp("guarded_" + name), sanitized=False)["plain"]
            for name, util in (("viterbi", viterbi_util), ("posterior", posterior_util), ("em", em_util), ("pairs", pairs_util))}


def exact_chain(hml, T, K):
    """a chain after three sweeps whose every position is a block (one position: the context with B = 1, as the tests of one
    block make it)"""
    from tests import test_gpu_em as te
    if T == 1:
        g = hml.Chain(device=0, seed=12)
        g.load(np.array([0.3], np.float32))
        g.em_nig4 = np.array([2.0, 1.0, 0.0, 1.0], np.float32)
        g.set_model(K, g.em_nig4)
        g.sample_prior()
        g.create_blocks(1.0)
    else:
        g = te.chain(hml, ol.trace(max(T, 16), min(K, 5), 4)[:T].copy(), K, every_position=True)
    assert g.num_blocks() == T
    return g


def same_trace(trace, want):
    return same_words(pu.words(trace), want)


def set_geometry(g, L, W, rounds):
    for pass_ in ("viterbi", "posterior"):
        g.set_option(pass_ + "_L", L)
        g.set_option(pass_ + "_W", W)
        g.set_option(pass_ + "_rounds", rounds)


@pytest.mark.parametrize("K", [2, 5, 16])
@pytest.mark.parametrize("T", EXACT_LENGTHS)
def test_exact_inference_at_full_capacity(guarded, programs, T, K):
    """viterbi, posterior, posterior_rle, expected_counts, posterior_breaks and posterior_regions under chunks of 4 and 64 blocks,
    warm-ups of 1 and 4, no repair round and 8: the words of the restatements, which do not know the geometry; then em_fit, without
    and with the prior, under the same eight"""
    from tests import em_util as eu
    from tests import pairs_util as pz
    from tests import test_gpu_em as te
    from tests import test_gpu_pairs as tp
    from tests import test_gpu_posterior as tpo
    from tests import test_gpu_viterbi as tv
    hml = guarded
    g = exact_chain(hml, T, K)
    what = "T = %d, %d states" % (T, K)
    case = pu.chain_case(g)
    want_v = tv.reference(programs["viterbi"], g)
    want_p = tpo.reference(programs["posterior"], g)
    want_e = eu.run_program(programs["em"], "estep", case)
    start, end = pz.edge_regions(case["starts"], np.random.default_rng(T), 20)
    start = np.concatenate([np.array([0, T - 1, 0], start.dtype), start])
    end = np.concatenate([np.array([1, T, T], end.dtype), end])
    want_r = pz.run_program(programs["pairs"], case, start, end)
    for L, W, rounds in GEOMETRIES:
        set_geometry(g, L, W, rounds)
        geo = (what, L, W, rounds)
        tv.check_decode(g, want_v, geo)
        tpo.check_results(g, want_p, geo)
        got = eu.chain_counts_words(g.expected_counts())
        for key in eu.COUNT_KEYS + ("loglik",):
            assert np.array_equal(got[key], want_e[key]), (geo, key)
        assert got["degenerate"] == want_e["degenerate"] and got["xi_degenerate"] == want_e["xi_degenerate"], geo
        terms = tp.terms_words(g.posterior_pair_terms())
        for key in pz.WORD_KEYS:
            assert np.array_equal(terms[key], want_r[key].ravel()), (geo, key)
        tp.check_breaks(g, want_r, case["starts"], geo)
        r = g.posterior_regions(start, end, raw=True)
        assert r["pair_degenerate"] == want_r["pair_degenerate"], geo
        pz.same_regions(pz.region_words(r), want_r, geo)
    # the tables of the decode and of the smoothing (scores, e, m, alpha, c, beta), the refusals of the regions
    tv.check(programs["viterbi"], g, what=what)
    tpo.check(programs["posterior"], g, what=what)
    tp.check(hml, programs["pairs"], g, what=what, n_random=20)
    # the fit: the restatement's trace and parameters (which do not know the geometry either), from the same start under all eight
    mv, (A, pi) = g.theta(), g.transitions()
    want_fit = {prior_on: eu.run_program(programs["em"], "fit", case, use_prior=prior_on, prior=te.prior(g), max_steps=3) for prior_on in (False, True)}
    for L, W, rounds in GEOMETRIES:
        set_geometry(g, L, W, rounds)
        for prior_on, want in want_fit.items():
            geo = (what, L, W, rounds, prior_on)
            g.set_parameters(mv, A, pi)
            trace, steps, reason, kept = g.em_fit(3, use_prior=prior_on)
            assert same_trace(trace, want["trace"]), (geo, trace, want["trace"].view(np.float64))
            assert (steps, reason, kept) == (want["steps"], want["reason"], want["kept"]), geo
            A2, pi2 = g.transitions()
            assert np.array_equal(pu.words32(g.theta()), want["mean_var"]) and np.array_equal(pu.words32(A2), want["A"]) and np.array_equal(pu.words32(pi2), want["pi"]), geo
    clean(hml)
    g.close()


@pytest.mark.parametrize("K", [2, 5, 16])
@pytest.mark.parametrize("T", [1, 2, 5, 64, 65, 1025])
def test_em_from_five_starts_at_full_capacity(guarded, programs, T, K):
    """em_fit_many over five starts, in one group (the default budget) and in groups of one (a budget of one byte): every member
    is its twin - set_parameters + em_fit - and members 0 and 4 are the restatement's fit, word for word"""
    from tests import em_util as eu
    from tests import test_gpu_em as te
    from tests import test_gpu_em_many as tm
    g = exact_chain(guarded, T, K)
    starts = g.em_starts(5, 7)
    case = pu.chain_case(g)
    for n_bytes, groups in ((0, 1), (1, 5)):
        g.set_em_batch_bytes(n_bytes)
        what = (T, K, n_bytes)
        got = tm.check_batch(g, starts, max_steps=3, use_prior=T == 1, what=what)      # every member against its twin
        info = g.em_many_info()
        assert (info["members"], info["groups"]) == (5, groups), info
        for r in (0, 4):
            m = tm.member_words(got, r)
            want = eu.run_program(programs["em"], "fit", dict(case, mean_var=starts[0][r], A=starts[1][r], pi=starts[2][r]), use_prior=T == 1,
                                  prior=te.prior(g), max_steps=3)
            assert same_words(np.asarray(m["trace"], np.uint64), np.asarray(want["trace"], np.uint64)), (what, r, got["trace"][r], want["trace"].view(np.float64))
            assert (m["steps"], m["reason"], m["kept"]) == (want["steps"], want["reason"], want["kept"]), (what, r)
            for key in ("mean_var", "A", "pi"):
                assert same_words(np.asarray(m[key], np.uint32), np.asarray(want[key], np.uint32), 32), (what, r, key)
    clean(guarded)
    g.close()


# ------------------------------------------------------------------------------------------------ e. recorders
@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("T", gu.RECORDER_LENGTHS)
def test_recorders_at_full_capacity(guarded, T, D):
    """the hand-made record of tests/guarded_util.record_all: two data dimensions with 31 band edges - the 64 columns the bands hold
    at most - and three with 20"""
    from tests import readout_fuzz_util as rf
    c = gu.record_all(T, D=D)
    exp = rf.expectations(c)
    reg = list(zip(exp["regions"][0].tolist(), exp["regions"][1].tolist()))
    assert (0, 1) in reg and (T - 1, T) in reg and (0, T) in reg
    assert len(exp["chains"][0]["rows"]) == 36 > 32
    assert all(len(s[0]) == T + 1 for per_token in exp["chains"][0]["sweeps"] for s in per_token), "every position a block"
    assert rf.run_configuration(guarded, c) == "ok"


def test_history_buffer_grows_twice(guarded):
    """The 36 rows of the record above are meant to cross the history buffer's capacity twice.  The growth count is no read-out, but
    what the library holds is: over four calls of nine sweeps, every sweep a row, the bytes it holds rise in at least two of the last
    three (hml_history_ensure doubles the buffer: 16 rows, 32, 64) - the rows of the old buffer are copied into recycled, poisoned
    memory - and the 36 rows are all there, in order, none dropped; the chain is the checker's."""
    hml = guarded
    o, g = full_chain(hml, 65, 5, scheme=[])
    g.set_history(True, 1)
    g.sample_prior()
    held = []
    for call in range(4):
        o.iterate("F", 9, 0)
        g.iterate("F", 9, 0)
        g.sync()
        held.append(hml.device_memory_live()[0])
        assert np.array_equal(g.history()[:, 0], np.arange(1, 9 * (call + 1) + 1)), call
    assert sum(b > a for a, b in zip(held, held[1:])) >= 2, held
    assert g.history_dropped() == 0
    compare_state(o, g, what="the chain whose history grew")
    clean(hml)
    g.close()
    o.close()


# ------------------------------------------------------------------------------------------------ h. caller-given device memory
MARGIN = 4096     # elements on either side of the view


def into_a_view(call, rows, T, dtype, sentinel):
    """`call(ptr)` writes [rows][T] elements of dtype: once into a tensor of exactly that size, once into the inside of a larger one
    whose margins hold the sentinel.  The margins stay, nothing of the sentinel is left inside, both results are the same bytes.
    Returns the result."""
    n = rows * T
    exact = torch.full((n,), sentinel, dtype=dtype, device="cuda:0")
    big = torch.full((n + 2 * MARGIN,), sentinel, dtype=dtype, device="cuda:0")
    torch.cuda.synchronize()          # (the fills run on torch's stream, the read-outs on the chain's)
    call(exact.data_ptr())
    call(big[MARGIN:MARGIN + n].data_ptr())
    torch.cuda.synchronize()
    big_h, exact_h = big.cpu().numpy(), exact.cpu().numpy()
    assert np.all(big_h[:MARGIN] == sentinel) and np.all(big_h[MARGIN + n:] == sentinel), "a store outside the caller's buffer"
    inside = big_h[MARGIN:MARGIN + n]
    assert not np.any(inside == sentinel) and not np.any(exact_h == sentinel), "an element of the caller's buffer was not written"
    assert inside.tobytes() == exact_h.tobytes()
    return exact_h.reshape(rows, T)


@pytest.mark.parametrize("T,D", gu.VIEW_CASES)
def test_dense_read_outs_into_a_view_of_a_larger_tensor(guarded, monkeypatch, T, D):
    """hml_marginals_dense_device, hml_levels_dense_device, hml_breaks_dense_device, hml_bands_dense_device and
    hml_levels_agreement_dense_device: first each dense form against its run-length form, which is held against the checker
    (tests/readout_fuzz_util.check_chain, check_dense), then into the inside of a larger tensor.  One data dimension: two chains
    of a batch, for the agreement; two dimensions: one chain of four states."""
    from tests import readout_fuzz_util as rf
    hml = guarded
    c = gu.view_record(T, D)
    for k in rf.ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    exp = rf.expectations(c)
    gs = rf._gpu_chains(hml, c, exp)
    try:
        for tok in c["scheme"]:
            rf._run_token(hml, c, gs, tok)
        for chain, g in enumerate(gs):
            rf.check_chain(hml, g, c, exp, chain, "chain %d" % chain)
        g, K = gs[0], c["K"]
        for pick in range(4):      # marginals, levels, breaks, bands
            rf.check_dense(hml, g, dict(c, dense_pick=pick), exp, 0, "dense form %d" % pick)
        nb = len(c["band_edges"][1]) + 1
        into_a_view(g.marginals_dense_device, K + 1, T, torch.int32, -7)
        into_a_view(lambda p: g.marginals_dense_device(p, g.relabel_permutation()), K + 1, T, torch.int32, -7)
        into_a_view(g.levels_dense_device, 2 * c["D"], T, torch.float32, -7.0)
        for window in (0, 1, 16):
            into_a_view(lambda p: g.breaks_dense(p, window), 1, T, torch.float32, -7.0)
        for cumulative in (False, True):
            into_a_view(lambda p: g.bands_dense_device(p, cumulative), c["D"] * nb, T, torch.int32, -7)
        if len(gs) > 1:
            into_a_view(lambda p: hml.levels_agreement_dense_device(gs, p), c["D"], T, torch.float32, -7.0)
        clean(hml)
    finally:
        for g in reversed(gs):
            g.close()


def test_agreement_of_one_position_into_a_view_of_a_larger_tensor(guarded):
    """hml_levels_agreement_dense_device at T = 1, which the records above cannot reach (the automatic prior refuses one observation
    of one dimension): two attached chains under the fixed prior of tests/test_gpu_forward_loads.set_up, each the checker's chain;
    the dense form is the run-length form's R-hat rounded once, inside a larger tensor as in one of its size"""
    from tests import test_gpu_agreement as ta
    hml = guarded
    T, K = 1, 3
    x = ol.trace(2, K, 7)[:T]
    pairs = []
    for chain in range(2):
        o = ol.OracleChain(K=K, seed=9, chain=chain, rng=ol.RNG_CTR, math=ol.MATH_DEV, reduce=ol.REDUCE_DEV, weight_mult=1e9)
        o.load(x)
        g = hml.Chain(device=0, seed=9, chain_id=chain)
        if chain == 0:
            g.load(x)
            g.scale_weights(1e9)
        else:
            g.attach(pairs[0][1])
        set_up(o, g, x, K)
        g.set_level_recording(True)
        o.token("F")
        g.sample_prior()
        o.set_record(marginals=True)
        pairs.append((o, g))
    gs = [g for _, g in pairs]
    for o, _ in pairs:
        o.iterate("F", 6, 1)
    hml.iterate_many(gs, "F", 6, 1)
    for chain, (o, g) in enumerate(pairs):
        g.sync()
        check(hml, o, g, T, "attached chain %d of 2, one position" % chain)
    seg, n, _, _, rhat = ta.assert_agreement(hml, gs, "one position")
    assert n == 6 and list(seg) == [1]
    dense = into_a_view(lambda p: hml.levels_agreement_dense_device(gs, p), 1, T, torch.float32, -7.0)
    assert np.array_equal(dense.view(np.uint32), np.repeat(rhat.astype(np.float32), seg.astype(np.int64), axis=1).view(np.uint32))
    clean(hml)
    for o, g in reversed(pairs):
        g.close()
        o.close()


# ------------------------------------------------------------------------------------------------ i. the driver
def test_driver_writes_the_same_files_under_the_mode(hml, tmp_path, monkeypatch):
    """every output of `hammlet` at once, two chains on one GPU, with HML_GUARD_BYTES = 4096 and HML_POISON = 1 in the child's
    environment alone: the files of the run without them, byte for byte, and no line of a damaged guard on stderr"""
    from tests import cli_util
    from tests.test_gpu_cli import ALL_OUTPUTS
    x = ol.trace(20000, 3, 9)
    files = {}
    for mode in ("plain", "guarded"):
        tmp = str(tmp_path / mode)
        os.mkdir(tmp)
        regions = os.path.join(tmp, "regions.txt")
        with open(regions, "w") as f:
            f.write("100 200 first\n5000 20000\n")
        flags = "-s 3 -R 4 -i F 4 0 F 6 2 -bands -0.5 0.5 -regions %s -em 3 -em-starts 2 -history-skip 0 -chains 2" % regions
        with monkeypatch.context() as m:
            m.delenv("HML_GUARD_BYTES", raising=False)
            m.delenv("HML_POISON", raising=False)
            if mode == "guarded":
                m.setenv("HML_GUARD_BYTES", str(gu.GUARD_BYTES))
                m.setenv("HML_POISON", "1")
            r = cli_util.run_cli(tmp, x, flags, list(ALL_OUTPUTS), one_gpu=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert hml.GUARD_TAG not in r.stderr, r.stderr
        files[mode] = {f: open(os.path.join(tmp, f), "rb").read() for f in sorted(os.listdir(tmp)) if f.startswith("g-")}
    assert len(files["plain"]) >= 20 and sorted(files["plain"]) == sorted(files["guarded"])
    for name, content in files["plain"].items():
        assert files["guarded"][name] == content, name

"""The two count tables of a chain - state marginals and level bands - read out in all three forms and compared with each
other in numpy: run-length segments (hml_marginals_rle, hml_bands_rle), dense tables (hml_marginals_dense_device,
hml_bands_dense_device) and calls compressed to runs (hml_max_segmentation, hml_bands_call at rank 0).  The forms share one
host path (hml_readout.hip: table_segments, table_rle, table_dense, table_runs); the cases put the number of segments M at
the edges of that path's kernels - one segment, one chunk of 256 segments, several chunks with a ragged tail - and T at the
ragged ends of the bitmap word (32) and of the dense kernels' chunk (4096).  Everything is integers: every comparison is exact.
What the counts ARE is the business of test_gpu_parity.py, test_gpu_maxseg.py and test_gpu_bands.py (against the checker)."""
import numpy as np
import pytest

from tests import hostile_inputs as hi
from tests import oracle_lib as ol

pytestmark = pytest.mark.gpu


def _noisy(T):
    """four integer levels that change at every position: every position a block, a run start and a band change"""
    return (10 * (hi._hash(T, 5) % 4)).astype(np.float32) + ol.trace(T, 3, 2)


def _two_dims(T):
    return np.stack([ol.trace(T, 2, 9 + d) for d in range(2)], axis=1).reshape(-1)


REGIMES = {
    "one": lambda M: M == 1,                          # only position 0
    "chunk": lambda M: 2 <= M <= 256,                 # one chunk of the segment kernels
    "ragged": lambda M: M > 256 and M % 256 != 0,     # several chunks, the last one partly filled
}

# name -> T, K, (D, P), seed, scheme, observations, band edges, regime of M (both tables)
CASES = {
    # (the seed: the two positions share their state in each of the ten recorded sweeps; the edge lies above every level)
    "one_segment": dict(T=2, K=2, D=1, P=None, seed=23, scheme=[("F", 10, 1)], x=lambda: hi.data("tiny_2"), edges=(1e30,), regime="one"),
    "one_chunk": dict(T=5000, K=3, D=1, P=None, seed=4, scheme=[("F", 12, 2)], x=lambda: ol.trace(5000, 3, 7), edges=(-0.5, 0.5), regime="chunk"),
    "ragged_k20": dict(T=6001, K=20, D=1, P=None, seed=3, scheme=[("F", 8, 1)], x=lambda: _noisy(6001), edges=(5.0, 15.0, 25.0), regime="ragged"),
    "two_dims": dict(T=4500, K=4, D=2, P=2, seed=6, scheme=[("M", 3, 1), ("F", 9, 2)], x=lambda: _two_dims(4500), edges=(0.0,), regime="chunk"),
}


def test_cases_cover_the_edges():
    cs = CASES.values()
    assert {c["regime"] for c in cs} == set(REGIMES)
    assert any(c["T"] % 32 for c in cs)
    assert any(c["T"] > 4096 and c["T"] % 4096 for c in cs)
    assert any(c["K"] > 16 for c in cs)                       # hml_k_seg_argmax<HML_CAP_K>
    assert any(c["D"] == 2 for c in cs)                       # two digits in hml_k_bands_pick's key


def expand(seg_len, counts):
    """run-length rows [M][ncol] -> dense [ncol][T]"""
    return np.repeat(counts, seg_len.astype(np.int64), axis=0).T


def start_indicator(seg_len, T):
    ind = np.zeros(T, np.int32)
    ind[np.cumsum(seg_len.astype(np.int64)) - seg_len.astype(np.int64)] = 1
    return ind


def first_maximum(rows):
    """the arg-max of every column of rows[n][T]: first maximum, strict `>` starting from count 0 (hml_k_seg_argmax)"""
    best = np.zeros(rows.shape[1], np.int64)
    best_count = np.zeros(rows.shape[1], np.int64)
    for s in range(rows.shape[0]):
        better = rows[s] > best_count
        best[better] = s
        best_count[better] = rows[s][better]
    return best


def runs(key):
    """(lengths, first positions) of the runs of equal neighbours in key[T]"""
    first = np.flatnonzero(np.r_[True, key[1:] != key[:-1]])
    return np.diff(np.r_[first, key.size]), first


@pytest.mark.parametrize("name", sorted(CASES))
def test_three_forms_of_both_tables_agree(hml, name):
    import torch
    c = CASES[name]
    T, K, D = c["T"], c["K"], c["D"]
    nb = len(c["edges"]) + 1
    g = hml.Chain(device=0, seed=c["seed"])
    if D > 1:
        g.set_dimensions(D, c["P"])
    g.load(c["x"]())
    g.set_model(K, g.autoprior(0.2, 0.9))
    g.set_level_bands(c["edges"])
    g.sample_prior()
    for tok in c["scheme"]:
        g.iterate(*tok)
    g.sync()
    N = g.recorded_sweeps()
    assert N == sum(n // t for _, n, t in c["scheme"] if t)

    # ---- state marginals
    seg, cnt = g.marginals_rle()
    M = len(seg)
    print("%s: marginals M = %d in %d columns, N = %d" % (name, M, cnt.shape[1], N))
    assert REGIMES[c["regime"]](M), (name, "marginals", M)
    assert int(seg.sum()) == T and np.all(seg > 0)
    assert np.all(cnt.sum(axis=1) == N)
    want = np.zeros((K + 1, T), np.int32)
    want[:cnt.shape[1]] = expand(seg, cnt)
    want[K] = start_indicator(seg, T)
    out = torch.full((K + 1, T), -7, dtype=torch.int32, device="cuda:0")
    g.marginals_dense_device(out.data_ptr())
    assert np.array_equal(out.cpu().numpy(), want), name
    perm = np.arange(K, dtype=np.int32)[::-1].copy()
    out.fill_(-7)
    g.marginals_dense_device(out.data_ptr(), perm)
    assert np.array_equal(out.cpu().numpy(), want[np.r_[perm, K]]), name
    run_len, run_state = g.max_segmentation()
    want_len, first = runs(first_maximum(want[:K]))
    assert int(run_len.sum()) == T
    assert np.array_equal(run_len.astype(np.int64), want_len) and np.array_equal(run_state, first_maximum(want[:K])[first]), name

    # ---- level bands
    bseg, bcnt, bN = g.bands_rle()
    bM = len(bseg)
    print("%s: bands M = %d in %d columns" % (name, bM, bcnt.shape[1]))
    assert REGIMES[c["regime"]](bM), (name, "bands", bM)
    assert bN == N and bcnt.shape == (bM, D * nb)
    assert int(bseg.sum()) == T and np.all(bseg > 0)
    for d in range(D):
        assert np.all(bcnt[:, d * nb:(d + 1) * nb].sum(axis=1) == N)
    bwant = expand(bseg, bcnt).astype(np.int32)
    bout = torch.full((D * nb, T), -7, dtype=torch.int32, device="cuda:0")
    g.bands_dense_device(bout.data_ptr())
    assert np.array_equal(bout.cpu().numpy(), bwant), name
    # rank 0 (hml_k_bands_pick): per dimension the band with the largest count, first maximum, strict `>` from count 0;
    # segments merge where the calls of ALL dimensions agree
    call = np.stack([first_maximum(bwant[d * nb:(d + 1) * nb]) for d in range(D)])
    key = sum(call[d] * nb ** d for d in range(D))
    want_len, first = runs(key)
    run_len, run_band = g.bands_call(0)
    assert int(run_len.sum()) == T and run_band.shape == (D, len(want_len))
    assert np.array_equal(run_len.astype(np.int64), want_len) and np.array_equal(run_band, call[:, first]), name
    g.close()

"""TEST INFRASTRUCTURE: the agreement of chains on the emission level (include/hml.h, hml_levels_agreement_rle) restated in
numpy from per-chain run-length levels - what `Chain.levels_rle()` returns, or tests/levels_util.py's accumulator cut into
segments - and, independently of any segments, position by position from dense per-chain sums.
"""
import numpy as np

from hammlet_amd import capi


def starts_of(seg_len):
    seg_len = np.asarray(seg_len, np.int64)
    return np.cumsum(seg_len) - seg_len


def union_starts(seg_lens):
    """the union of the chains' segment starts, ascending (position 0 is in every chain's)"""
    return np.unique(np.concatenate([starts_of(s) for s in seg_lens]))


def onto_union(seg_len, values, union):
    """values[..., M] of a chain's own segments repeated onto the union's segments: the segment that contains each union start"""
    idx = np.searchsorted(starts_of(seg_len), union, side="right") - 1
    return np.asarray(values)[..., idx]


def agreement_from_rle(chains_rle, T):
    """chains_rle: per chain (seg_len[M], N, s1[D, M], s2[D, M]).  Returns (union seg_len[U], within[D, U], between[D, U],
    rhat[D, U]) by capi.levels_rhat on the chains' values repeated onto the union."""
    N = chains_rle[0][1]
    assert all(c[1] == N for c in chains_rle)
    union = union_starts([c[0] for c in chains_rle])
    s1 = np.stack([onto_union(c[0], c[2], union) for c in chains_rle])
    s2 = np.stack([onto_union(c[0], c[3], union) for c in chains_rle])
    within, between, rhat = capi.levels_rhat(N, s1, s2)
    return np.diff(np.append(union, T)), within, between, rhat


def agreement_dense(N, S1, S2):
    """Brute force: S1, S2 of shape [n][D][T], the chains' sums at every position.  The same formula, written out again
    position by position (not through capi.levels_rhat): (within, between, rhat), [D][T] each."""
    S1 = np.asarray(S1, np.float64)
    S2 = np.asarray(S2, np.float64)
    n = S1.shape[0]
    Nf = np.float64(N)
    sum_q = np.zeros(S1.shape[1:], np.float64)
    sum_m = np.zeros(S1.shape[1:], np.float64)
    for c in range(n):
        m = S1[c] / Nf
        q = S2[c] / Nf - m * m
        q[~(q > 0.0)] = 0.0
        sum_q = sum_q + q
        sum_m = sum_m + m
    w0 = sum_q / np.float64(n)
    mbar = sum_m / np.float64(n)
    sum_b = np.zeros(S1.shape[1:], np.float64)
    for c in range(n):
        dev = S1[c] / Nf - mbar
        sum_b = sum_b + dev * dev
    between = sum_b / np.float64(n - 1)
    within = w0 * (Nf / (Nf - 1.0))
    rhat = np.empty_like(within)
    pos = within > 0.0
    rhat[pos] = np.sqrt((w0[pos] + between[pos]) / within[pos])
    rhat[~pos & (between == 0.0)] = 1.0
    rhat[~pos & (between > 0.0)] = np.inf
    return within, between, rhat


def rle_of_dense(S1, S2, boundary):
    """a chain's dense sums [D, T] and boundary indicator as run-length levels: (seg_len, s1[D, M], s2[D, M])"""
    pos = np.flatnonzero(boundary)
    return np.diff(np.append(pos, len(boundary))), S1[:, pos], S2[:, pos]


def bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def ulps64(a, b):
    """distance in units of the last place between float64 arrays of finite, positive values (and 0 where both are +inf)"""
    a = np.ascontiguousarray(a, np.float64)
    b = np.ascontiguousarray(b, np.float64)
    d = np.abs(a.view(np.int64) - b.view(np.int64))
    return d

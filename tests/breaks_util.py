"""TEST INFRASTRUCTURE: breakpoint posteriors and the consensus segmentation (include/hml.h, hml_breaks_*) restated in numpy.

Input: one (starts, states, mean_per_parameter) per recorded sweep - what `blocks()`, `states()` and the even entries of
`theta()` of the CPU checker return after that sweep, as in tests/levels_util.py.  A sweep has a breakpoint at t iff a block
b > 0 starts at t with states[b] != states[b - 1].  Everything here is written for clarity, not speed: the consensus is
the brute-force O(M * window) rule, the dense form a windowed sum by prefix sums over all T positions.
"""
import math

import numpy as np

from tests import levels_util as lu


def sweep_breaks(starts, states):
    """positions of the breakpoints of one sweep"""
    starts = np.asarray(starts, np.int64)
    states = np.asarray(states, np.int64)
    change = np.zeros(len(states), bool)
    change[1:] = states[1:] != states[:-1]
    return starts[:-1][change]


def counts(sweeps, T):
    """(C[T] int64, N)"""
    C = np.zeros(T, np.int64)
    for starts, states, _ in sweeps:
        pos = sweep_breaks(starts, states)
        assert np.all(pos > 0) and np.all(pos < T)
        C[pos] += 1
    return C, len(sweeps)


def listing(C):
    """(positions with C > 0 ascending, their counts)"""
    pos = np.flatnonzero(C)
    return pos, C[pos]


def windowed(C, window):
    """W[t] = sum of C[u] over |u - t| <= window, int64"""
    T = len(C)
    pre = np.concatenate([[0], np.cumsum(C)])
    t = np.arange(T, dtype=np.int64)
    return pre[np.minimum(t + window + 1, T)] - pre[np.maximum(t - window, 0)]


def dense(C, N, window):
    """float32 [T]: windowed(C) / N, the quotient in double, rounded once; N = 0: NaN"""
    if N == 0:
        return np.full(len(C), np.nan, np.float32)
    return (windowed(C, window).astype(np.float64) / np.float64(N)).astype(np.float32)


def consensus(C, window, min_count):
    """brute force: (pos, mass, peak) of the selected candidates, and per candidate (mass, beaten by a neighbour?)"""
    pos, cnt = listing(C)
    need = max(int(min_count), 1)
    sel, mass_all, beaten_all = [], [], []
    T = len(C)
    for i in range(len(pos)):
        t, c = int(pos[i]), int(cnt[i])
        a, b = max(0, t - window), min(T - 1, t + window)
        near = C[a:b + 1]                      # every position of the window, candidates or not
        u = np.arange(a, b + 1)
        mass = int(near.sum())
        beaten = bool(np.any((u != t) & (near > 0) & ((near > c) | ((near == c) & (u < t)))))
        mass_all.append(mass)
        beaten_all.append(beaten)
        if mass >= need and not beaten:
            sel.append(i)
    sel = np.asarray(sel, np.int64)
    mass_all = np.asarray(mass_all, np.int64)
    return (pos[sel], mass_all[sel], cnt[sel]), (mass_all, np.asarray(beaten_all, bool))


def consensus_profile(C, window, min_count):
    """what makes a consensus case non-vacuous: numbers of selected, suppressed-by-a-neighbour and below-min_count candidates"""
    (pos, _, _), (mass, beaten) = consensus(C, window, min_count)
    need = max(int(min_count), 1)
    return {"selected": len(pos), "suppressed": int(np.sum(beaten & (mass >= need))), "below": int(np.sum(mass < need))}


def min_count_of(P, N):
    """the driver's rule: max(1, ceil(P * N)) in double"""
    return max(1, int(math.ceil(float(P) * float(N))))


def segment_sums(S, cuts):
    """sum over the positions of each of the len(cuts) + 1 segments of every row of S[D, T]; long double accumulation, so the
    reference's own summation error is below that of one double rounding"""
    T = S.shape[1]
    edges = np.concatenate([[0], np.asarray(cuts, np.int64), [T]])
    out = np.empty((S.shape[0], len(edges) - 1), np.float64)
    for d in range(S.shape[0]):
        pre = np.concatenate([[0], np.cumsum(S[d].astype(np.longdouble))])
        out[d] = (pre[edges[1:]] - pre[edges[:-1]]).astype(np.float64)
    return out, np.diff(edges)


def cuts_inside_fine_segments(boundary, cuts):
    """how many cuts fall strictly inside a fine level segment (are not a boundary of the levels)"""
    return int(np.sum(~np.asarray(boundary, bool)[np.asarray(cuts, np.int64)]))


def segment_bounds(M, N, mu_max, T, seg_len):
    """The arithmetic's bound on a sum of hml_levels_on_segments over a segment of seg_len positions (DESIGN.md 3c''):
       seg_len * E1                      the error of the levels' own sums (levels_util.bounds), once per position;
       2^-52 (depth + 4) T (N max + E1)  the roundings of length x value, of the fixed-shape scan a result passes through
                                         (depth = 23 + ceil(M / 2^20) additions), of the partial fine segment at either end
                                         and of the final difference - each at most 2^-53 of a partial sum, which is at
                                         most T (N max + E1) in magnitude; 2^-52 covers the second-order terms;
       seg_len * 2^-53 N^2 max           the expected value's own error: N additions per position in lu.accumulate.
    Returns (bound for S1, bound for S2) as arrays over the segments."""
    E1, E2 = lu.bounds(M, N, mu_max)
    depth = 23 + (M + (1 << 20) - 1) // (1 << 20)
    L = np.asarray(seg_len, np.float64)
    out = []
    for E, m in ((E1, mu_max), (E2, mu_max * mu_max)):
        out.append(L * E + 2.0 ** -52 * (depth + 4) * T * (N * m + E) + L * 2.0 ** -53 * N * N * m)
    return out[0], out[1]

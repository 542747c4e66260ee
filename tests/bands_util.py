"""TEST INFRASTRUCTURE: the level bands per position (include/hml.h, hml_set_level_bands / hml_bands_rle / hml_bands_call)
restated in numpy.

Input: one (starts, states, mean_per_parameter) per recorded sweep - what `blocks()`, `states()` and the even entries of
`theta()` of a chain return after that sweep - plus the edges, D and P.  The level of dimension d under a block in state s is
mean[(s // P**d) % P]; its band is the number of edges <= the level, compared as float32 (np.searchsorted, side="right"; a
level that is not a number: band 0).  Dense int64 counts [D * (n_edges + 1)][T] by plain per-sweep addition; a segment
boundary lies where the band of any dimension changes between adjacent positions of a sweep, united over the sweeps.
Nothing here comes from the product.
"""
import math

import numpy as np

from tests import levels_util as lu


def band_of(edges, mean):
    edges = np.asarray(edges, np.float32)
    mean = np.asarray(mean, np.float32)
    b = np.searchsorted(edges, mean, side="right")
    return np.where(np.isnan(mean), 0, b).astype(np.int64)


def sweep_bands(sweep, edges, D=1, P=None):
    """(run start positions, bands[D, runs]) of one sweep's runs of equal STATE"""
    starts, states, mean = sweep
    mean = np.asarray(mean, np.float32)
    Pn = P if P is not None else len(mean)
    pos, st = lu.run_starts(starts, states)
    band_of_param = band_of(edges, mean)
    return pos, np.stack([band_of_param[(st // Pn ** d) % Pn] for d in range(D)], axis=0)


def accumulate(sweeps, T, edges, D=1, P=None):
    """(counts[D * nb, T] int64, boundary[T] bool, N)"""
    nb = len(edges) + 1
    counts = np.zeros((D * nb, T), np.int64)
    boundary = np.zeros(T, bool)
    boundary[0] = True
    for sweep in sweeps:
        pos, bands = sweep_bands(sweep, edges, D, P)
        length = np.diff(np.append(pos, T))
        dense = np.repeat(bands, length, axis=1)          # [D, T]
        for d in range(D):
            counts[d * nb + dense[d], np.arange(T)] += 1
        boundary[1:] |= np.any(dense[:, 1:] != dense[:, :-1], axis=0)
    return counts, boundary, len(sweeps)


def rle(counts, boundary):
    """(segment lengths[M], counts[M, columns]) - the shape of hml_bands_rle"""
    pos, length = lu.segments(boundary)
    return length, np.ascontiguousarray(counts[:, pos].T)


def cumulative(counts, D, nb):
    """row b of dimension d: the sweeps in band b or above"""
    c = counts.reshape(D, nb, -1)
    return np.cumsum(c[:, ::-1], axis=1)[:, ::-1].reshape(D * nb, -1)


def exceedance(seg_counts, n_edges, D):
    """per segment and edge: the sweeps whose level was >= the edge (what capi.bands_exceedance must give)"""
    nb = n_edges + 1
    out = np.zeros((len(seg_counts), D * n_edges), np.int64)
    for d in range(D):
        for j in range(n_edges):
            out[:, d * n_edges + j] = seg_counts[:, d * nb + j + 1:(d + 1) * nb].sum(axis=1)
    return out


def call(seg_counts, length, rank, D, nb):
    """(run_len[R], run_band[D, R]): rank 0 - the band with the largest count, first maximum; rank >= 1 - the smallest band
    whose cumulative count over the bands up to it reaches rank; adjacent segments that agree in every dimension merged"""
    seg_counts = np.asarray(seg_counts, np.int64)
    M = len(seg_counts)
    bands = np.zeros((D, M), np.int64)
    for d in range(D):
        c = seg_counts[:, d * nb:(d + 1) * nb]
        if rank == 0:
            bands[d] = np.argmax(c, axis=1)               # (the first maximum; all zero: band 0)
        else:
            reached = np.cumsum(c, axis=1) >= rank
            assert np.all(reached[:, -1]), "rank beyond the recorded sweeps"
            bands[d] = np.argmax(reached, axis=1)
    first = np.ones(M, bool)
    first[1:] = np.any(bands[:, 1:] != bands[:, :-1], axis=0)
    start = np.concatenate([[0], np.cumsum(length)[:-1]])[first]
    return np.diff(np.append(start, int(np.sum(length)))), bands[:, first]


def rank_of(p, N):
    """the driver's rule for -bandcall P"""
    return 0 if p == 0 or N == 0 else min(N, max(1, int(math.ceil(p * N))))


def level_segments(sweeps, T):
    """number of the levels' segments: boundaries between runs of different STATES, united over the sweeps"""
    boundary = np.zeros(T, bool)
    boundary[0] = True
    for starts, states, _ in sweeps:
        boundary[lu.run_starts(starts, states)[0]] = True
    return int(boundary.sum())


def bands_text(length, seg_counts):
    """PREFIXbandsSUFFIX: the marginals file's shape"""
    return "".join("\t".join([str(int(l))] + [str(int(v)) for v in row]) + "\n" for l, row in zip(length, seg_counts))


def calls_text(run_len, run_band):
    """PREFIXbandcallsSUFFIX: start length band_0 [band_1 ...]"""
    start = np.concatenate([[0], np.cumsum(run_len)[:-1]])
    return "".join(" ".join([str(int(s)), str(int(l))] + [str(int(b)) for b in run_band[:, r]]) + "\n"
                   for r, (s, l) in enumerate(zip(start, run_len)))

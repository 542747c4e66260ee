"""TEST INFRASTRUCTURE: the emission levels per position (include/hml.h, hml_levels_rle) restated in numpy.

Input: one (starts, states, mean_per_parameter) per recorded sweep - what `blocks()`, `states()` and the even entries of
`theta()` of a chain return after that sweep - plus D and P.  The level of dimension d under a block in state s is
mean[(s // P**d) % P].  Dense float64 sums by plain per-sweep addition; the run boundaries are those between adjacent
blocks of different STATE (the marginals' rule), united over the sweeps.
"""
import numpy as np


def param_of_state(K, D, P):
    """[K, D]: the emission parameter state s uses for dimension d (the mapping of hml_set_dimensions)"""
    s = np.arange(K)
    return np.stack([(s // P ** d) % P for d in range(D)], axis=1)


def run_starts(starts, states):
    """(positions where a run of equal states starts, the state of each run)"""
    starts = np.asarray(starts, np.int64)
    states = np.asarray(states, np.int64)
    first = np.ones(len(states), bool)
    first[1:] = states[1:] != states[:-1]
    return starts[:-1][first], states[first]


def accumulate(sweeps, T, D=1, P=None, value=None):
    """sweeps: list of (starts[B + 1], states[B], mean[P]).  Returns (S1[D, T], S2[D, T], boundary[T] bool, N).
    `value(sweep index, d, run states) -> float64 per run` replaces the level (the checker's validation feeds an indicator)."""
    S1 = np.zeros((D, T), np.float64)
    S2 = np.zeros((D, T), np.float64)
    boundary = np.zeros(T, bool)
    boundary[0] = True
    for n, (starts, states, mean) in enumerate(sweeps):
        mean = np.asarray(mean, np.float32)
        Pn = P if P is not None else len(mean)
        pos, st = run_starts(starts, states)
        boundary[pos] = True
        length = np.diff(np.append(pos, T))
        for d in range(D):
            if value is not None:
                v = np.asarray(value(n, d, st), np.float64)
            else:
                v = mean[(st // Pn ** d) % Pn].astype(np.float64)
            dense = np.repeat(v, length)
            S1[d] += dense
            S2[d] += dense * dense
    return S1, S2, boundary, len(sweeps)


def segments(boundary):
    """(segment starts, segment lengths) of a boundary indicator"""
    pos = np.flatnonzero(boundary)
    return pos, np.diff(np.append(pos, len(boundary)))


def max_abs_mean(sweeps):
    """max |mu| over the theta of all recorded sweeps (0 if there are none)"""
    return max([float(np.max(np.abs(np.asarray(m, np.float64)))) for _, _, m in sweeps] + [0.0])


def bounds(M, N, mu_max):
    """The arithmetic's error bounds of a segment sum: at most N rounded additions of terms of at most
    2 max into each cell, then at most M rounded additions in the scan.  E1 for the level, E2 for its square."""
    e = 2.0 ** -52 * M * N * (N + 1)
    return e * mu_max, e * mu_max * mu_max

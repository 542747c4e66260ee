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


# ---- the device's double sums restated bit for bit (hml_levels_rle, hml_levels_merge, hml_levels_on_segments) ----
# Not a bound but the very additions, in the device's order: every function below is plain elementwise float64 numpy (the
# library is built without fused multiply-adds), so equal bits are the expectation.

def exact_cells(sweeps, T, D=1, P=None):
    """The difference cells of one chain: (acc[2 D, T] float64, boundary[T] bool).  A cell starts at +0.0 and receives, in
    sweep order, mn - mp (row 2 d) and mn*mn - mp*mp (row 2 d + 1) where a run of equal states starts: mn, mp the float32
    means of the run's state and of the run before it (0.0 before the first), widened to float64."""
    acc = np.zeros((2 * D, T), np.float64)
    boundary = np.zeros(T, bool)
    boundary[0] = True
    for starts, states, mean in sweeps:
        mean = np.asarray(mean, np.float32).astype(np.float64)
        Pn = P if P is not None else len(mean)
        pos, st = run_starts(starts, states)
        boundary[pos] = True
        for d in range(D):
            mn = mean[(st // Pn ** d) % Pn]
            mp = np.concatenate(([0.0], mn[:-1]))
            acc[2 * d, pos] = acc[2 * d, pos] + (mn - mp)
            acc[2 * d + 1, pos] = acc[2 * d + 1, pos] + (mn * mn - mp * mp)
    return acc, boundary


def exact_merge(dst, src):
    """hml_levels_merge: the source's cells are added, each as one number, to the destination's at the source's boundaries"""
    (acc_d, bnd_d), (acc_s, bnd_s) = dst, src
    acc = acc_d.copy()
    acc[:, bnd_s] = acc_d[:, bnd_s] + acc_s[:, bnd_s]
    return acc, bnd_d | bnd_s


def _guarded_doubling(a):
    """Hillis-Steele over the last axis: in step d (1, 2, 4, ...) entry i >= d becomes a[i] + a[i - d]; entries below d are
    left alone (not `+ 0.0`)"""
    a = a.copy()
    d = 1
    while d < a.shape[-1]:
        nxt = a.copy()
        nxt[..., d:] = a[..., d:] + a[..., :-d]
        a = nxt
        d *= 2
    return a


def exact_scan(x):
    """Inclusive sums of x[M] over the device's fixed tree: chunks of 1024; in a chunk four sequential additions per thread
    from 0.0, eight guarded doubling steps over the 256 threads' sums, and thread i > 0 adds the sum of thread i - 1 in front
    of its four; the chunk totals in 1024 pieces of ceil(chunks / 1024), each summed sequentially from 0.0, ten guarded
    doubling steps over the pieces, and piece i > 0 runs on from the sum of piece i - 1 (`part[i - 1]`, not `part[i] - sum`);
    last, `base + v` per entry."""
    x = np.asarray(x, np.float64)
    M = x.size
    n_chunks = (M + 1023) // 1024
    pad = np.zeros(n_chunks * 1024, np.float64)
    pad[:M] = x
    live = (np.arange(n_chunks * 1024) < M).reshape(n_chunks, 256, 4)
    pad = pad.reshape(n_chunks, 256, 4)
    v = np.empty_like(pad)
    run = np.zeros((n_chunks, 256), np.float64)
    for k in range(4):
        run = np.where(live[:, :, k], run + pad[:, :, k], run)
        v[:, :, k] = run
    sh = _guarded_doubling(run)
    v[:, 1:, :] = sh[:, :-1, None] + v[:, 1:, :]
    total = v[:, 255, 3]
    # exclusive sums of the chunk totals
    per = (n_chunks + 1023) // 1024
    cs = np.zeros(1024 * per, np.float64)
    cs[:n_chunks] = total
    live_c = (np.arange(1024 * per) < n_chunks).reshape(1024, per)
    cs = cs.reshape(1024, per)
    s = np.zeros(1024, np.float64)
    for j in range(per):
        s = np.where(live_c[:, j], s + cs[:, j], s)
    part = _guarded_doubling(s)
    run = np.concatenate(([0.0], part[:-1]))
    base = np.empty_like(cs)
    for j in range(per):
        base[:, j] = run
        run = np.where(live_c[:, j], run + cs[:, j], run)
    base = base.reshape(-1)[:n_chunks]
    return (base[:, None, None] + v).reshape(-1)[:M]


def exact_rle(cells):
    """what hml_levels_rle returns for the cells of exact_cells / exact_merge: (segment starts[M], sums[2 D, M])"""
    acc, boundary = cells
    pos = np.flatnonzero(boundary)
    return pos, np.stack([exact_scan(row[pos]) for row in acc])


def exact_on_segments(cells, cuts):
    """what hml_levels_on_segments returns, rows as in exact_cells: out[2 D, len(cuts) + 1].  w_i = len_i * v_i, the same tree
    over w, F(x) = pw[lo - 1] + (x - start[lo]) * v[lo] (without the first term for lo = 0; pw[M - 1] for x = T), F(b) - F(a)."""
    acc, boundary = cells
    T = boundary.size
    pos, v = exact_rle(cells)
    M = pos.size
    length = np.diff(np.append(pos, T)).astype(np.float64)
    edges = np.concatenate(([0], np.asarray(cuts, np.int64), [T]))
    lo = np.searchsorted(pos, np.minimum(edges, T - 1), side="right") - 1
    out = np.empty((acc.shape[0], edges.size - 1), np.float64)
    for r in range(acc.shape[0]):
        pw = exact_scan(length * v[r])
        part = (edges - pos[lo]).astype(np.float64) * v[r][lo]
        F = np.where(lo > 0, pw[np.maximum(lo, 1) - 1] + part, part)
        F = np.where(edges >= T, pw[M - 1], F)
        out[r] = F[1:] - F[:-1]
    return out


# Chains on which the exact restatement is compared (tests/test_gpu_levels.py), chosen on the CPU checker so that the number
# of segments M lands in every structural regime of the tree; tests/test_levels_cpu.py asserts the ranges without a GPU.
# name: (trace, T, K, seed, [(chain id, scheme), ...] - more than one: merged into the first -, (least M, most M))
EXACT_CASES = {
    "nothing_recorded": ("levels", 50000, 3, 11, [(0, [("F", 20, 50)])], (1, 1)),                         # thinning beyond the sweeps
    "one_partial_chunk": ("depth", 900, 5, 17, [(0, [("M", 4, 0), ("F", 6, 2)])], (2, 1023)),
    "several_chunks": ("depth", 4000, 5, 17, [(0, [("M", 4, 0), ("F", 6, 2)])], (2049, 4095)),            # the last one partial
    "pieces_of_two_chunks": ("depth", 4000000, 5, 17, [(0, [("M", 1, 1), ("F", 2, 1)])], ((1 << 20) + 1, 1 << 21)),
    "merged_pair": ("depth", 4000, 5, 17, [(0, [("M", 4, 0), ("F", 6, 2)]), (1, [("M", 2, 1), ("F", 4, 2)])], (2049, 4095)),
}


def exact_case_trace(name):
    from tests import oracle_lib as ol
    kind, T, K = EXACT_CASES[name][:3]
    return ol.synth_depth(T, seed=5) if kind == "depth" else ol.trace(T, K, 7)


def exact_case_cells(name, sweeps_per_chain):
    """The cells of a case from the recorded sweeps of each of its chains (merged into the first), with the assertions that
    make the case mean something: M in its range, not a multiple of the chunk, and a merge that adds boundaries."""
    T = EXACT_CASES[name][1]
    lo, hi = EXACT_CASES[name][5]
    per_chain = [exact_cells(sweeps, T) for sweeps in sweeps_per_chain]
    cells = per_chain[0]
    for other in per_chain[1:]:
        assert np.any(other[1] & ~cells[1]) and np.any(cells[1] & ~other[1]), name   # each side has boundaries of its own
        cells = exact_merge(cells, other)
    M = int(cells[1].sum())
    assert lo <= M <= hi, (name, M, lo, hi)
    assert M == 1 or M % 1024 != 0, (name, M)
    return cells


def exact_case_cuts(name, cells):
    """cuts for hml_levels_on_segments: on segment starts, beside them, and the two extreme positions"""
    T = EXACT_CASES[name][1]
    pos = np.flatnonzero(cells[1])
    pick = pos[:: max(1, pos.size // 40)]
    cuts = np.concatenate(([1, T - 1], pick, pick + 1, np.arange(T // 7, T, T // 7)))
    return np.unique(cuts[(cuts > 0) & (cuts < T)]).astype(np.uint32)

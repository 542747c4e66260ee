"""TEST INFRASTRUCTURE: the joint posteriors over regions (include/hml.h, hml_set_regions / hml_regions_read) restated in numpy.

Input: one (starts[B + 1], states[B], mean_per_parameter) per recorded sweep - what `blocks()`, `states()` and the even entries
of `theta()` of a chain return after that sweep - plus the regions [a, e), the edges, D and P.  With blk(p) the last block that
starts at or before p, ba = blk(a), be = blk(e - 1):
  nb     the blocks b in (ba, be] with states[b] != states[b - 1]                       (cumsum + searchsorted, exact)
  same_d the band of dimension d (bands_util.band_of over the regions' own edges) does not change in (ba, be]; j_d = that of ba
  m_d    (F_d(e) - F_d(a)) / (e - a), F_d(p) = the level of dimension d summed over the positions below p, in np.longdouble
         (64 bits of mantissa: asserted below), so the reference's own error is 2^-11 of the bound the doubles are held to.
Nothing here comes from the product.

The bound (DESIGN.md 3c''''''), for ANY order of the double additions: with m = max |mean| over the recorded thetas and, per
sweep s of B_s blocks, e_s = 2 (B_s + 4) 2^-53 T m / len:
  |level_sum error| <= sum_s e_s + N^2 2^-53 m,       |level_sq error| <= sum_s (2 m e_s + e_s^2) + (N^2 + N) 2^-53 m^2.
"""
import numpy as np

from tests import bands_util as bu

assert np.finfo(np.longdouble).nmant >= 63, "the reference needs an extended-precision long double"

U64_MAX = 2 ** 64 - 1
KEYS = ("whole", "breaks_sum", "breaks_sq", "level_sum", "level_sq", "inband")


def sweep_values(sweep, start, end, edges=(), D=1, P=None):
    """(nb[R] int64, m[D, R] longdouble, same[D, R] bool, band[D, R] int64) of one sweep"""
    starts, states, mean = sweep
    starts = np.asarray(starts, np.int64)
    states = np.asarray(states, np.int64)
    mean32 = np.asarray(mean, np.float32)
    Pn = P if P is not None else len(mean32)
    a, e = np.asarray(start, np.int64), np.asarray(end, np.int64)
    B = len(states)
    assert len(starts) == B + 1 and starts[0] == 0 and np.all(a < e) and np.all(e <= starts[-1])
    ba = np.searchsorted(starts[:-1], a, side="right") - 1
    be = np.searchsorted(starts[:-1], e - 1, side="right") - 1

    def changes_inside(values):
        ch = np.zeros(B + 1, np.int64)                 # ch[k + 1] = changes at the blocks 1 .. k
        ch[2:] = np.cumsum(values[1:] != values[:-1])
        return ch[be + 1] - ch[ba + 1]

    nb = changes_inside(states)
    length = np.diff(starts).astype(np.longdouble)
    band_of_param = bu.band_of(edges, mean32) if len(edges) else np.zeros(len(mean32), np.int64)
    m = np.zeros((D, len(a)), np.longdouble)
    same = np.zeros((D, len(a)), bool)
    band = np.zeros((D, len(a)), np.int64)
    for d in range(D):
        param = (states // Pn ** d) % Pn
        level = mean32[param].astype(np.longdouble)    # (a float converts exactly)
        F = np.concatenate([[np.longdouble(0)], np.cumsum(length * level)])

        def below(p, b):                               # the level summed over the positions below p, p in block b (or its end)
            return F[b] + (p - starts[b]).astype(np.longdouble) * level[b]
        m[d] = (below(e, be) - below(a, ba)) / (e - a).astype(np.longdouble)
        bands = band_of_param[param]
        same[d] = changes_inside(bands) == 0
        band[d] = bands[ba]
    return nb, m, same, band


def accumulate(sweeps, start, end, edges=(), D=1, P=None):
    """dict(N, whole, breaks_sum, breaks_sq (python ints in object arrays are avoided: uint64 with the saturation rule),
    level_sum, level_sq [D, R] longdouble, inband [R, D * (n_edges + 1)] uint64, bound_sum, bound_sq [R] float64)"""
    R = len(start)
    nbands = len(edges) + 1
    ncol = D * nbands if len(edges) else 0
    out = dict(N=len(sweeps), whole=np.zeros(R, np.uint64), breaks_sum=np.zeros(R, np.uint64), breaks_sq=np.zeros(R, np.uint64),
               level_sum=np.zeros((D, R), np.longdouble), level_sq=np.zeros((D, R), np.longdouble), inband=np.zeros((R, ncol), np.uint64))
    for sweep in sweeps:
        nb, m, same, band = sweep_values(sweep, start, end, edges, D, P)
        out["whole"] += (nb == 0).astype(np.uint64)
        out["breaks_sum"] += nb.astype(np.uint64)
        out["breaks_sq"] = sat_add(out["breaks_sq"], (nb * nb).astype(np.uint64))      # (nb < 2^32: one term never overflows)
        out["level_sum"] += m
        out["level_sq"] += m * m
        for d in range(D if ncol else 0):
            r = np.flatnonzero(same[d])
            out["inband"][r, d * nbands + band[d][r]] += np.uint64(1)
    out["bound_sum"], out["bound_sq"] = bounds(sweeps, start, end)
    return out


def sat_add(a, b):
    """uint64 addition that saturates at 2^64 - 1 and stays there"""
    a, b = np.asarray(a, np.uint64), np.asarray(b, np.uint64)
    s = a + b                                           # (wraps)
    return np.where(s < a, np.uint64(U64_MAX), s)


def bounds(sweeps, start, end):
    """(bound of |level_sum error|, bound of |level_sq error|) per region, from T, B_s, N, m and len alone"""
    length = (np.asarray(end, np.float64) - np.asarray(start, np.float64))
    N = len(sweeps)
    if N == 0:
        return np.zeros(len(length)), np.zeros(len(length))
    m = max(float(np.max(np.abs(np.asarray(s[2], np.float64)))) for s in sweeps)
    u = 2.0 ** -53
    b_sum = np.zeros(len(length))
    b_sq = np.zeros(len(length))
    for starts, states, _ in sweeps:
        T = float(starts[-1])
        e_s = 2.0 * (len(states) + 4) * u * T * m / length
        b_sum += e_s
        b_sq += 2.0 * m * e_s + e_s * e_s
    return b_sum + N * N * u * m, b_sq + (N * N + N) * u * m * m


def assert_matches(got, want, what=""):
    """a chain's regions() against the helper's: integers exactly, doubles under the bound (printed next to the largest error)"""
    assert got["N"] == want["N"], (what, got["N"], want["N"])
    for k in ("whole", "breaks_sum", "breaks_sq", "inband"):
        assert got[k].dtype == np.uint64 and got[k].shape == want[k].shape, (what, k, got[k].shape, want[k].shape)
        assert np.array_equal(got[k], want[k]), (what, k, np.flatnonzero(np.any(np.atleast_2d(got[k].T != want[k].T), axis=0))[:8])
    for k, bound in (("level_sum", want["bound_sum"]), ("level_sq", want["bound_sq"])):
        assert got[k].dtype == np.float64 and got[k].shape == want[k].shape, (what, k)
        err = np.abs(got[k].astype(np.longdouble) - want[k]).astype(np.float64)
        worst = np.unravel_index(np.argmax(err - bound[None, :]), err.shape)
        print("%s: %s largest error %.3e (bound there %.3e, smallest bound %.3e)" % (what, k, err.max(), bound[worst[1]], bound.min()))
        assert np.all(err <= bound[None, :]), (what, k, worst, err[worst], bound[worst[1]])


def standard_regions(T, last_sweep, seed=0, n_random=300):
    """The regions of every GPU case: the whole trace, its first and last position, one-position regions on a block start of
    the checker's last sweep, one before and one after it, a region strictly inside a block, a duplicate, a nested pair and
    `n_random` random ones of mixed lengths - shuffled.  (start, end) as uint32."""
    starts = np.asarray(last_sweep[0], np.int64)
    rng = np.random.RandomState(seed)
    reg = [(0, T), (0, 1), (T - 1, T)]
    inner = starts[1:-1]
    if len(inner):
        s = int(inner[len(inner) // 2])
        reg += [(s, s + 1), (s - 1, s), (s + 1, s + 2), (s - 1, s + 1)]
    size = np.diff(starts)
    wide = np.flatnonzero(size >= 3)
    if len(wide):
        b = int(wide[len(wide) // 2])
        reg.append((int(starts[b]) + 1, int(starts[b + 1]) - 1))
    reg += [(T // 3, T // 2), (T // 3, T // 2)]                       # a duplicate
    reg += [(T // 4, 3 * T // 4 + 1), (T // 4 + T // 8, T // 2 + 1)]   # a nested pair
    for _ in range(n_random):
        length = int(min(T, 10 ** rng.uniform(0, 4.5)))
        a = int(rng.randint(0, T - length + 1))
        reg.append((a, a + max(1, length)))
    reg = [(a, e) for a, e in reg if 0 <= a < e <= T]
    order = rng.permutation(len(reg))
    reg = np.asarray(reg, np.int64)[order]
    return reg[:, 0].astype(np.uint32), reg[:, 1].astype(np.uint32)


# ---- chunk edges: traces on which every position is a block (test_regions_cpu.py asserts the block counts on the checker) ----
# the kernels take blocks in chunks of 256 and a wavefront has 64 lanes: B = 63, 64, 65, 255, 256, 257, and 1023 / 1024 blocks
# (four chunks, the last one short of a block / full); B = 2 the smallest
EDGE_B = {2: 2, 63: 63, 64: 64, 65: 65, 255: 255, 256: 256, 257: 257, 1024: 1023, 1025: 1024}      # T -> B of every sweep
EDGE_SCHEME = [("F", 6, 1)]


def edge_case(T):
    from tests import oracle_lib as ol
    return dict(T=T, K=3, seed=5, scheme=EDGE_SCHEME, trace=ol.trace(T, 3, 7) * np.float32(1024), D=1, P=None, compat=False, env={},
                edges=(-512.0, 512.0))


def edge_regions(T, seed=0):
    """every region of a short trace (T <= 65); else regions that begin or end at, one before and one after the chunk and
    wavefront edges, plus a few hundred random ones"""
    if T <= 65:
        a, e = np.triu_indices(T + 1, 1)
        return a.astype(np.uint32), e.astype(np.uint32)
    reg = []
    for x in (63, 64, 65, 255, 256, 257, 511, 512, 513, 767, 768, 769, 1023, 1024):
        for y in (x - 1, x, x + 1):
            if 0 < y < T:
                reg += [(0, y), (y, T), (y - 1, y), (y, y + 1), (max(0, y - 256), y), (y, min(T, y + 256)), (max(0, y - 3), min(T, y + 3))]
    rng = np.random.RandomState(seed)
    a = rng.randint(0, T, size=300)
    e = np.minimum(T, a + 1 + rng.randint(0, T, size=300))
    b = rng.randint(0, T - 4, size=200)                  # (short ones: whole in some sweeps, cut in others)
    reg = np.asarray(reg + list(zip(a, e)) + list(zip(b, b + rng.randint(2, 5, size=200))), np.int64)
    reg = reg[rng.permutation(len(reg))]
    return reg[:, 0].astype(np.uint32), reg[:, 1].astype(np.uint32)


# ---- the driver's files ----
def regions_file_text(start, end, labels=None):
    """a -regions FILE: "start end [label]" per line, behind a comment and a blank line"""
    lines = ["# start end label", ""]
    for r in range(len(start)):
        lines.append("%d %d%s" % (start[r], end[r], (" " + labels[r]) if labels is not None and labels[r] else ""))
    return "\n".join(lines) + "\n"


def parse_output(text, D, ncol):
    """PREFIXregionsSUFFIX: per line start, end, N, whole, breaks mean and sd, per d level mean and sd, inband per column, label -
    tab-separated.  dict of arrays (the means and spreads as printed: float32 through %.9g)"""
    rows = [line.split("\t") for line in text.splitlines()]
    width = 6 + 2 * D + ncol + 1
    assert all(len(r) == width for r in rows), [len(r) for r in rows if len(r) != width][:4]
    col = lambda j, t: np.array([t(r[j]) for r in rows])
    return dict(start=col(0, int), end=col(1, int), N=col(2, int), whole=col(3, int), breaks_mean=col(4, float), breaks_sd=col(5, float),
                level_mean=np.stack([col(6 + 2 * d, float) for d in range(D)]), level_sd=np.stack([col(7 + 2 * d, float) for d in range(D)]),
                inband=np.stack([col(6 + 2 * D + j, int) for j in range(ncol)], axis=1) if ncol else np.zeros((len(rows), 0), int),
                label=[r[-1] for r in rows])


# malformed -regions files over an input of 2000 positions: (text, what the driver's message says); None: no such file
MALFORMED = [
    ("10 5\n", "the end (5) must lie beyond the start (10)"),
    ("10 10 gene\n", "the end (10) must lie beyond the start (10)"),
    ("0 2001\n", "the end (2001) lies beyond the 2000 positions of the input"),
    ("0 x\n", 'two whole numbers, found "x"'),
    ("-3 7\n", 'two whole numbers, found "-3"'),
    ("1.5 7\n", 'two whole numbers, found "1.5"'),
    ("12\n", "found one number only"),
    ("# only a comment\n\n   \n", "holds no regions"),
    ("", "holds no regions"),
    (None, "Cannot read from regions file"),
]


def write_malformed(folder, text):
    """the file of a MALFORMED case, a good region in front of a bad line; returns its name"""
    import os
    fn = os.path.join(folder, "regions.txt")
    if text is not None:
        with open(fn, "w") as f:
            f.write(regions_file_text([0, 5], [10, 2000], ["a", ""]) + text if text.strip() and not text.startswith("#") else text)
    return fn

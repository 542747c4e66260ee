"""TEST INFRASTRUCTURE: the pairwise read-outs of the smoothing (hml_posterior_breaks, hml_posterior_regions,
hml_posterior_pair_terms of include/hml.h) restated in Python floats and integers in the order hammlet_amd/csrc/hml_pairs_ref.h
uses, behind the smoothing restatement of tests/posterior_util.py; an enumeration of all K^B paths; and the plumbing of the
stand-alone program tests/fixtures/pairs_ref_main.cpp.  Doubles are compared as their 64-bit words, the fixed-point values as
integers."""
import itertools
import math
import os
import subprocess

import numpy as np

from tests import posterior_util as pu
from tests.posterior_util import _d2u, _hex, _u2d, bad, chain_case, hml_log, words   # noqa: F401

REPO = pu.REPO
SRC = os.path.join(REPO, "tests", "fixtures", "pairs_ref_main.cpp")
CAP = 1023 * 2 ** 22
TWO32 = 4294967296.0
TWO22 = 4194304.0


def build_programs(directory, sanitized=True):
    """the plain build (-Wall -Werror) and, if asked, the sanitizer build of the stand-alone program: name -> path"""
    out = {}
    kinds = [("plain", ["-O2"])]
    if sanitized:
        kinds.append(("sanitized", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]))
    for name, extra in kinds:
        exe = os.path.join(str(directory), "pairs_" + name)
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off"] + extra + ["-o", exe, SRC], check=True)
        out[name] = exe
    return out


def case_text(case, start=(), end=()):
    B = len(case["starts"]) - 1
    head = "pairs %d %d %d %d %d %d" % (case["K"], case["D"], case["P"], 1 if case["self_trans"] else 0, B, len(start))
    return "\n".join([head, " ".join(map(str, np.asarray(case["starts"]).tolist())), _hex(case["sum"]), _hex(case["sum_sq"]), _hex(case["mean_var"]),
                      _hex(case["A"]), _hex(case["pi"]), " ".join(map(str, np.asarray(start).tolist())), " ".join(map(str, np.asarray(end).tolist()))]) + "\n"


_PER_K = ("r", "cost", "mass", "gamma", "whole_state", "share")
WORD_KEYS = ("p", "r", "pfx", "cost", "mass")
REGION_KEYS = ("whole", "whole_state", "expected_breaks", "share", "raw")


def run_program(exe, case, start=(), end=()):
    """the program's words: every array as uint64 (doubles as their words), per-state arrays as [., K], raw as [n, 2 K + 1]"""
    r = subprocess.run([exe], input=case_text(case, start, end), capture_output=True, text=True)
    assert r.stderr == "", r.stderr                     # (the sanitizers report there)
    assert r.returncode == 0, (r.returncode, r.stdout[:200])
    K = case["K"]
    out = {}
    for line in r.stdout.splitlines():
        name, _, rest = line.partition(" ")
        if name == "seconds":
            out[name] = float(rest)
        elif name == "pair_degenerate":
            out[name] = int(rest)
        elif name == "total":
            out[name] = int(rest, 16)
        else:
            out[name] = np.array([int(v, 16) for v in rest.split()], np.uint64)
    for name in _PER_K:
        out[name] = out[name].reshape(-1, K)
    out["raw"] = out["raw"].reshape(-1, 2 * K + 1)
    return out


# ---- the definition, in Python floats and integers ----
def hml_exp_nonpos(x):
    """hml_exp_nonpos of hammlet_amd/csrc/hml_math.h, operation by operation"""
    ln2_hi, ln2_lo = 6.93147180369123816490e-01, 1.90821492927058770002e-10
    invln2 = 1.44269504088896338700e+00
    P1, P2, P3 = 1.66666666666666019037e-01, -2.77777777770155933842e-03, 6.61375632143793436117e-05
    P4, P5 = -1.65339022054652515390e-06, 4.13813679705723846039e-08
    if not (x <= 0.0):
        return x if x != x else 1.0
    if x < -700.0:
        return 0.0
    shift = 6755399441055744.0
    kd = x * invln2 + shift
    k = (_d2u(kd) & 0xFFFFFFFFFFFFF) - 0x8000000000000
    kd = kd - shift
    hi = x - kd * ln2_hi
    lo = kd * ln2_lo
    r = hi - lo
    rr = r * r
    c = r - rr * (P1 + rr * (P2 + rr * (P3 + rr * (P4 + rr * P5))))
    y = 1.0 - ((lo - (r * c) / (2.0 - c)) - hi)
    return y * _u2d((k + 1023) << 52)


def _div(a, b):
    """IEEE division of Python floats (no exception for a zero divisor)"""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def fx32(g):
    """llrint(g 2^32): the product is exact, round() is to nearest, ties to even"""
    return round(g * TWO32)


def cost_of(u, r):
    if bad(u) or not (r > 0.0):
        return CAP
    nl = -hml_log(r)
    nl = nl if nl > 0.0 else 0.0
    return min(round(nl * TWO22), CAP)


def terms(case):
    """dict(p[B], r[B][K], pfx[B], cost[B][K], mass[B][K], gamma, alpha, beta, N[B], C[K][B], G[K][B] (Python floats and
    integers), pair_degenerate)"""
    K = case["K"]
    e_rows, m = pu.tables(case)
    s = pu.smooth(case, e_rows, m)
    B = len(e_rows)
    A = [[float(v) for v in row] for row in np.asarray(case["A"], np.float32).reshape(K, K)]
    e = [[float(v) for v in row] for row in e_rows]
    starts = [int(v) for v in case["starts"]]
    p, r, pfx, cost = [0.0], [[0.0] * K], [0], [[0] * K]
    degenerate = 0
    for b in range(1, B):
        v = [e[b][j] * s["beta"][b][j] for j in range(K)]
        d = o = 0.0
        for i in range(K):
            for j in range(K):
                x = (s["alpha"][b - 1][i] * A[i][j]) * v[j]
                if j == i:
                    d = d + x
                else:
                    o = o + x
        X = d + o
        deg = bad(X)
        degenerate += deg
        pb = 0.0 if deg else o / X
        p.append(pb)
        pfx.append(fx32(pb))
        rr, cc = [], []
        for j in range(K):
            u = 0.0
            for k in range(K):
                u = u + A[j][k] * v[k]
            q = 0.0 if bad(u) else _div(A[j][j] * v[j], u)
            rr.append(q)
            cc.append(cost_of(u, q))
        r.append(rr)
        cost.append(cc)
    mass = [[(starts[b + 1] - starts[b]) * fx32(s["gamma"][b][j]) for j in range(K)] for b in range(B)]
    N = list(itertools.accumulate(pfx))
    C = [list(itertools.accumulate(cost[b][j] for b in range(B))) for j in range(K)]
    G = [list(itertools.accumulate(mass[b][j] for b in range(B))) for j in range(K)]
    return dict(p=p, r=r, pfx=pfx, cost=cost, mass=mass, gamma=s["gamma"], alpha=s["alpha"], beta=s["beta"], N=N, C=C, G=G, pair_degenerate=degenerate)


def block_of(starts, pos):
    """the block that holds position pos"""
    return int(np.searchsorted(np.asarray(starts[:-1], np.int64), pos, side="right")) - 1


def region(case, t, start, end):
    """dict(whole, whole_state[K], expected_breaks, share[K], raw[2 K + 1], ba, be) of one region"""
    K = case["K"]
    starts = [int(v) for v in case["starts"]]
    ba, be = block_of(starts, start), block_of(starts, end - 1)
    nb = t["N"][be] - t["N"][ba]
    cut_a, cut_e = start - starts[ba], starts[be + 1] - end
    ws, share, dcs, ms = [], [], [], []
    whole = 0.0
    for j in range(K):
        ga, ge = t["gamma"][ba][j], t["gamma"][be][j]
        dc = t["C"][j][be] - t["C"][j][ba]
        w = ga * hml_exp_nonpos(-float(dc) * (1.0 / TWO22))
        ws.append(w)
        whole = whole + w
        m = t["G"][j][be] - (t["G"][j][ba - 1] if ba else 0) - cut_a * fx32(ga) - cut_e * fx32(ge)
        assert 0 <= m < 2 ** 64
        share.append((float(m) * (1.0 / TWO32)) / float(end - start))
        dcs.append(dc)
        ms.append(m)
    return dict(whole=whole, whole_state=ws, expected_breaks=float(nb) * (1.0 / TWO32), share=share, raw=[nb] + dcs + ms, ba=ba, be=be)


def regions(case, t, start, end):
    """the same for arrays of regions, in the shapes run_program() and Chain.posterior_regions() use"""
    rs = [region(case, t, int(a), int(e)) for a, e in zip(start, end)]
    K = case["K"]
    return dict(whole=np.array([r["whole"] for r in rs], np.float64), whole_state=np.array([r["whole_state"] for r in rs], np.float64).reshape(-1, K),
                expected_breaks=np.array([r["expected_breaks"] for r in rs], np.float64), share=np.array([r["share"] for r in rs], np.float64).reshape(-1, K),
                raw=np.array([r["raw"] for r in rs], np.uint64).reshape(-1, 2 * K + 1))


def enumerate_pairs(case):
    """all K^B paths (weights in double, sums by math.fsum): a function region(start, end) -> dict(whole_state, whole,
    expected_breaks, share), and p[B]; None if no path has weight"""
    K = case["K"]
    e_rows, _ = pu.tables(case)
    B = len(e_rows)
    A = np.asarray(case["A"], np.float32).reshape(K, K).astype(np.float64)
    pi = np.asarray(case["pi"], np.float32).astype(np.float64)
    starts = [int(v) for v in case["starts"]]
    paths, weights = [], []
    for path in itertools.product(range(K), repeat=B):
        w = float(pi[path[0]])
        for b, s in enumerate(path):
            w *= float(e_rows[b][s])
            if b:
                w *= float(A[path[b - 1], s])
        paths.append(path)
        weights.append(w)
    Z = math.fsum(weights)
    if Z == 0.0:
        return None
    p = [0.0] + [math.fsum(w for q, w in zip(paths, weights) if q[b] != q[b - 1]) / Z for b in range(1, B)]
    gamma = [[math.fsum(w for q, w in zip(paths, weights) if q[b] == j) / Z for j in range(K)] for b in range(B)]

    def of(start, end):
        ba, be = block_of(starts, start), block_of(starts, end - 1)
        ws = [math.fsum(w for q, w in zip(paths, weights) if all(q[b] == j for b in range(ba, be + 1))) / Z for j in range(K)]
        share = []
        for j in range(K):
            share.append(math.fsum((min(starts[b + 1], end) - max(starts[b], start)) * gamma[b][j] for b in range(ba, be + 1)) / (end - start))
        return dict(whole_state=ws, whole=math.fsum(ws), expected_breaks=math.fsum(p[ba + 1:be + 1]), share=share, ba=ba, be=be)

    return dict(p=p, gamma=gamma, region=of)


# ---- regions for a block structure ----
def edge_regions(starts, rng, n_random=0):
    """(start, end): one position, the whole trace, ends exactly on block starts and one position to either side, nested,
    overlapping and repeated regions, and n_random random ones"""
    starts = [int(v) for v in starts]
    T, B = starts[-1], len(starts) - 1
    rs = [(0, 1), (T - 1, T), (0, T), (0, T)]
    picks = sorted(set([1, B // 2, B - 1]) & set(range(1, B)))
    for b in picks:
        s = starts[b]
        for a in (s - 1, s, s + 1):
            for e in (s - 1, s, s + 1, T):
                if 0 <= a < e <= T:
                    rs.append((a, e))
            if 0 < a <= T:
                rs.append((0, a))
    if T >= 4:
        rs += [(T // 4, 3 * T // 4), (T // 4 + 1, T // 2), (T // 4, 3 * T // 4), (T // 2 - 1, T)]      # nested, repeated, overlapping
    if n_random:
        a = rng.integers(0, T, n_random)
        ln = np.minimum(rng.geometric(1.0 / max(2, T // 50), n_random), T - a)
        rs += list(zip(a.tolist(), (a + np.maximum(ln, 1)).tolist()))
    arr = np.array([r for r in rs if 0 <= r[0] < r[1] <= T], np.int64).reshape(-1, 2)
    return arr[:, 0].astype(np.uint32), arr[:, 1].astype(np.uint32)


# ---- comparing ----
def same_terms(got, want, what=None):
    """got: words (the program's, or chain_terms_words()); want: terms()"""
    for key in ("p", "r"):
        assert np.array_equal(np.asarray(got[key]).ravel(), words(np.array(want[key], np.float64))), (what, key)
    for key in ("pfx", "cost", "mass"):
        assert np.array_equal(np.asarray(got[key]).ravel(), np.array(want[key], np.uint64).ravel()), (what, key)


def region_words(r):
    """Chain.posterior_regions(raw=True), or regions(), as the program prints it"""
    return dict(whole=words(r["whole"]), whole_state=words(r["whole_state"]), expected_breaks=words(r["expected_breaks"]), share=words(r["share"]),
                raw=np.asarray(r["raw"], np.uint64).ravel())


def same_regions(got, want, what=None):
    """two dicts of words"""
    for key in REGION_KEYS:
        assert np.array_equal(np.asarray(got[key]).ravel(), np.asarray(want[key]).ravel()), (what, key)

"""TEST INFRASTRUCTURE: the count read-outs of the smoothing (hml_posterior_region_counts, hml_posterior_count_terms of
include/hml.h) restated in Python floats in the order hammlet_amd/csrc/hml_counts_ref.h uses, behind the smoothing restatement
of tests/posterior_util.py; an enumeration of all K^B paths that extends tests/pairs_util.enumerate_pairs with the histogram of
the number of breakpoints and the avoidance of a state; and the plumbing of the stand-alone program
tests/fixtures/counts_ref_main.cpp.  Doubles are compared as their 64-bit words."""
import itertools
import math
import os
import subprocess

import numpy as np

from tests import pairs_util as pz
from tests import posterior_util as pu
from tests.posterior_util import _hex, words   # noqa: F401

REPO = pu.REPO
SRC = os.path.join(REPO, "tests", "fixtures", "counts_ref_main.cpp")
U_MIN = 2.0 ** -1000
MAX_H = 32
MAX_CELLS = 1024
REGION_KEYS = ("hist", "whole_state", "avoid")


def h_ok(K, H):
    return 1 <= H <= MAX_H and K * (H + 1) <= MAX_CELLS


def build_programs(directory, sanitized=True):
    """the plain build (-Wall -Werror) and, if asked, the sanitizer build of the stand-alone program: name -> path"""
    out = {}
    kinds = [("plain", ["-O2"])]
    if sanitized:
        kinds.append(("sanitized", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]))
    for name, extra in kinds:
        exe = os.path.join(str(directory), "counts_" + name)
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off"] + extra + ["-o", exe, SRC], check=True)
        out[name] = exe
    return out


def case_text(case, start=(), end=(), H=8):
    B = len(case["starts"]) - 1
    head = "counts %d %d %d %d %d %d %d" % (case["K"], case["D"], case["P"], 1 if case["self_trans"] else 0, B, len(start), H)
    return "\n".join([head, " ".join(map(str, np.asarray(case["starts"]).tolist())), _hex(case["sum"]), _hex(case["sum_sq"]), _hex(case["mean_var"]),
                      _hex(case["A"]), _hex(case["pi"]), " ".join(map(str, np.asarray(start).tolist())), " ".join(map(str, np.asarray(end).tolist()))]) + "\n"


def run_program(exe, case, start=(), end=(), H=8):
    """the program's words: v, rho, gamma as uint64 [B, K]; hist [n, H + 1], whole_state and avoid [n, K] as uint64;
    count_degenerate, steps, longest as integers; seconds"""
    r = subprocess.run([exe], input=case_text(case, start, end, H), capture_output=True, text=True)
    assert r.stderr == "", r.stderr                     # (the sanitizers report there)
    assert r.returncode == 0, (r.returncode, r.stdout[:200])
    K = case["K"]
    out = {}
    for line in r.stdout.splitlines():
        name, _, rest = line.partition(" ")
        if name == "seconds":
            out[name] = float(rest)
        elif name in ("count_degenerate", "steps", "longest"):
            out[name] = int(rest)
        else:
            out[name] = np.array([int(v, 16) for v in rest.split()], np.uint64)
    for name in ("v", "rho", "gamma", "whole_state", "avoid"):
        out[name] = out[name].reshape(-1, K)
    out["hist"] = out["hist"].reshape(-1, H + 1)
    return out


# ---- the definition, in Python floats ----
def u_ok(u):
    return u >= U_MIN and u < math.inf


def v_kept(v):
    return v if (v >= 0.0 and v < math.inf) else 0.0


def terms(case):
    """dict(v[B][K], rho[B][K], gamma[B][K] (Python floats), A[K][K], count_degenerate)"""
    K = case["K"]
    e_rows, m = pu.tables(case)
    s = pu.smooth(case, e_rows, m)
    B = len(e_rows)
    A = [[float(x) for x in row] for row in np.asarray(case["A"], np.float32).reshape(K, K)]
    e = [[float(x) for x in row] for row in e_rows]
    v, rho = [[0.0] * K], [[0.0] * K]
    degenerate = 0
    for b in range(1, B):
        vb = [e[b][j] * s["beta"][b][j] for j in range(K)]
        rb = []
        for i in range(K):
            u = 0.0
            for k in range(K):
                u = u + A[i][k] * vb[k]
            ok = u_ok(u)
            degenerate += not ok
            rb.append(pz._div(1.0, u) if ok else 0.0)
        v.append([v_kept(x) for x in vb])
        rho.append(rb)
    return dict(v=v, rho=rho, gamma=s["gamma"], A=A, count_degenerate=degenerate)


def region(case, t, start, end, H):
    """dict(hist[H + 1], whole_state[K], avoid[K], ba, be) of one region"""
    K, A = case["K"], t["A"]
    starts = [int(x) for x in case["starts"]]
    ba, be = pz.block_of(starts, start), pz.block_of(starts, end - 1)
    ga = t["gamma"][ba]
    f = [[ga[j]] + [0.0] * H for j in range(K)]
    g = [[0.0 if i == x else ga[i] for i in range(K)] for x in range(K)]
    for b in range(ba + 1, be + 1):
        v, rho = t["v"][b], t["rho"][b]
        nf = []
        for j in range(K):
            row = []
            for h in range(H + 1):
                s = 0.0
                if h >= 1:
                    for i in range(K):
                        if i == j:
                            continue
                        src = f[i][h - 1] * rho[i]
                        if h == H:
                            src = src + f[i][h] * rho[i]
                        s = s + A[i][j] * src
                row.append((A[j][j] * (f[j][h] * rho[j]) + s) * v[j])
            nf.append(row)
        f = nf
        ng = []
        for x in range(K):
            row = []
            for i in range(K):
                s = 0.0
                for k in range(K):
                    if k != x:
                        s = s + A[k][i] * (g[x][k] * rho[k])
                row.append(0.0 if i == x else s * v[i])
            ng.append(row)
        g = ng
    hist = []
    for h in range(H + 1):
        s = 0.0
        for j in range(K):
            s = s + f[j][h]
        hist.append(s)
    avoid = []
    for x in range(K):
        s = 0.0
        for i in range(K):
            if i != x:
                s = s + g[x][i]
        avoid.append(s)
    return dict(hist=hist, whole_state=[f[j][0] for j in range(K)], avoid=avoid, ba=ba, be=be)


def regions(case, t, start, end, H):
    """the same for arrays of regions, in the shapes run_program() and Chain.posterior_region_counts() use"""
    rs = [region(case, t, int(a), int(e), H) for a, e in zip(start, end)]
    K = case["K"]
    return dict(hist=np.array([r["hist"] for r in rs], np.float64).reshape(-1, H + 1), whole_state=np.array([r["whole_state"] for r in rs], np.float64).reshape(-1, K),
                avoid=np.array([r["avoid"] for r in rs], np.float64).reshape(-1, K), steps=sum(r["be"] - r["ba"] for r in rs),
                longest=max([r["be"] - r["ba"] for r in rs], default=0))


def enumerate_counts(case):
    """all K^B paths (weights in double, sums by math.fsum): what tests/pairs_util.enumerate_pairs gives, and a function
    counts(start, end, H) -> dict(hist[H + 1], whole_state[K], avoid[K], ba, be); None if no path has weight"""
    base = pz.enumerate_pairs(case)
    if base is None:
        return None
    K = case["K"]
    e_rows, _ = pu.tables(case)
    B = len(e_rows)
    A = np.asarray(case["A"], np.float32).reshape(K, K).astype(np.float64)
    pi = np.asarray(case["pi"], np.float32).astype(np.float64)
    starts = [int(x) for x in case["starts"]]
    paths, weights = [], []
    for path in itertools.product(range(K), repeat=B):       # (the order and the weights of enumerate_pairs)
        w = float(pi[path[0]])
        for b, s in enumerate(path):
            w *= float(e_rows[b][s])
            if b:
                w *= float(A[path[b - 1], s])
        paths.append(path)
        weights.append(w)
    Z = math.fsum(weights)
    q = np.array(paths, np.int8).reshape(-1, B)
    w = np.array(weights, np.float64)
    changes = np.concatenate([np.zeros((len(q), 1), np.int64), np.cumsum(q[:, 1:] != q[:, :-1], axis=1)], axis=1)    # breakpoints up to block b

    def total(mask):
        return math.fsum(w[mask].tolist()) / Z      # (the selection is exact; the sum is fsum's)

    def of(start, end, H):
        ba, be = pz.block_of(starts, start), pz.block_of(starts, end - 1)
        n = changes[:, be] - changes[:, ba]
        hist = [total(np.minimum(n, H) == h) for h in range(H + 1)]
        whole = [total((n == 0) & (q[:, ba] == j)) for j in range(K)]
        avoid = [total(~(q[:, ba:be + 1] == x).any(axis=1)) for x in range(K)]
        return dict(hist=hist, whole_state=whole, avoid=avoid, ba=ba, be=be)

    return dict(base, counts=of)


# ---- comparing ----
def same_terms(got, want, what=None):
    """got: words [B, K] (the program's, or of Chain.posterior_count_terms()); want: terms()"""
    for key in ("v", "rho"):
        assert np.array_equal(np.asarray(got[key]).ravel(), words(np.array(want[key], np.float64))), (what, key)


def region_words(r):
    """Chain.posterior_region_counts(), or regions(), as the program prints it"""
    return {key: words(r[key]) for key in REGION_KEYS}


def same_regions(got, want, what=None):
    """two dicts of words"""
    for key in REGION_KEYS:
        a, b = np.asarray(got[key]).ravel(), np.asarray(want[key]).ravel()
        assert a.shape == b.shape, (what, key, a.shape, b.shape)
        if not np.array_equal(a, b):
            bad = np.flatnonzero(a != b)
            raise AssertionError((what, key, len(bad), int(bad[0]), hex(int(a[bad[0]])), hex(int(b[bad[0]]))))

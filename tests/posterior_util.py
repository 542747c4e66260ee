"""TEST INFRASTRUCTURE: the smoothing read-out of include/hml.h (hml_posterior) restated in Python - the float tables with
numpy float32 / Python float (IEEE double) arithmetic in the order hammlet_amd/csrc/hml_posterior_ref.h uses, the two normalised
recursions, the posteriors, the tree sum and the call, all in Python floats - an enumeration of all K^B paths, and the plumbing
of the stand-alone program tests/fixtures/posterior_ref_main.cpp.  Doubles are compared as their 64-bit words."""
import itertools
import math
import os
import struct
import subprocess

import numpy as np

from tests.viterbi_util import _hex, hml_log, hml_logf, make_case, chain_case, runs_of   # noqa: F401  (same cases, same logarithm)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "fixtures", "posterior_ref_main.cpp")
f32 = np.float32


def build_programs(directory, sanitized=True):
    """the plain build (-Wall -Werror) and, if asked, the sanitizer build of the stand-alone program: name -> path"""
    out = {}
    kinds = [("plain", ["-O2"])]
    if sanitized:
        kinds.append(("sanitized", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]))
    for name, extra in kinds:
        exe = os.path.join(str(directory), name)
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off"] + extra + ["-o", exe, SRC], check=True)
        out[name] = exe
    return out


def words(a):
    """float64 values as their uint64 words"""
    return np.ascontiguousarray(a, np.float64).ravel().view(np.uint64)


def words32(a):
    return np.ascontiguousarray(a, np.float32).ravel().view(np.uint32)


def case_text(case, want_rows=True):
    B = len(case["starts"]) - 1
    head = "case %d %d %d %d %d %d" % (case["K"], case["D"], case["P"], 1 if case["self_trans"] else 0, B, 1 if want_rows else 0)
    return "\n".join([head, " ".join(map(str, np.asarray(case["starts"]).tolist())), _hex(case["sum"]), _hex(case["sum_sq"]), _hex(case["mean_var"]),
                      _hex(case["A"]), _hex(case["pi"])]) + "\n"


def run_case(exe, case, want_rows=True):
    """the program's words: dict(m, e (uint32), alpha, c, beta, gamma, loglik, run_conf (uint64), degenerate, state, run_len, run_state, seconds)"""
    r = subprocess.run([exe], input=case_text(case, want_rows), capture_output=True, text=True)
    assert r.stderr == "", r.stderr                     # (the sanitizers report there)
    assert r.returncode == 0, (r.returncode, r.stdout[:200])
    K = case["K"]
    out = {}
    for line in r.stdout.splitlines():
        name, _, rest = line.partition(" ")
        if name == "seconds":
            out[name] = [float(v) for v in rest.split()]
        elif name == "degenerate":
            out[name] = int(rest)
        elif name in ("m", "e"):
            out[name] = np.array([int(v, 16) for v in rest.split()], np.uint32)
        elif name in ("alpha", "c", "beta", "gamma", "loglik", "run_conf"):
            out[name] = np.array([int(v, 16) for v in rest.split()], np.uint64)
        else:
            out[name] = np.array(rest.split(), np.int64)
    for name in ("e", "alpha", "beta", "gamma"):
        if name in out:
            out[name] = out[name].reshape(-1, K)
    return out


def random_case(rng, K, B, D=1, P=None, self_trans=True, max_len=5):
    """blocks of 1 ... max_len positions around random levels, random parameters, A and pi"""
    P = P or K
    lens = rng.integers(1, max_len + 1, B)
    starts = np.concatenate([[0], np.cumsum(lens)])
    level = rng.normal(0, 2, (D, B))
    sx = np.empty((D, B), np.float32)
    sq = np.empty((D, B), np.float32)
    for d in range(D):
        for b in range(B):
            x = rng.normal(level[d, b], 1.0, lens[b]).astype(np.float32)
            sx[d, b] = x.sum(dtype=np.float32)
            sq[d, b] = (x * x).sum(dtype=np.float32)
    mean = np.sort(rng.normal(0, 2, P)).astype(np.float32)
    var = rng.uniform(0.3, 2.0, P).astype(np.float32)
    mv = np.stack([mean, var], 1).ravel()
    A = rng.dirichlet(np.ones(K), K).astype(np.float32)
    pi = rng.dirichlet(np.ones(K)).astype(np.float32)
    return make_case(K, starts, sx, sq, mv, A, pi, D=D, P=P, self_trans=self_trans)


# ---- the float tables ----
_EXP2F_TAB = [
    0x3ff0000000000000, 0x3fefd9b0d3158574, 0x3fefb5586cf9890f, 0x3fef9301d0125b51, 0x3fef72b83c7d517b, 0x3fef54873168b9aa, 0x3fef387a6e756238,
    0x3fef1e9df51fdee1, 0x3fef06fe0a31b715, 0x3feef1a7373aa9cb, 0x3feedea64c123422, 0x3feece086061892d, 0x3feebfdad5362a27, 0x3feeb42b569d4f82,
    0x3feeab07dd485429, 0x3feea47eb03a5585, 0x3feea09e667f3bcd, 0x3fee9f75e8ec5f74, 0x3feea11473eb0187, 0x3feea589994cce13, 0x3feeace5422aa0db,
    0x3feeb737b0cdc5e5, 0x3feec49182a3f090, 0x3feed503b23e255d, 0x3feee89f995ad3ad, 0x3feeff76f2fb5e47, 0x3fef199bdd85529c, 0x3fef3720dcef9069,
    0x3fef5818dcfba487, 0x3fef7c97337b9b5f, 0x3fefa4afa2a490da, 0x3fefd0765b6e4540]


def _d2u(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def _u2d(u):
    return struct.unpack("<d", struct.pack("<Q", u))[0]


def hml_expf(x):
    """hml_expf of hammlet_amd/csrc/hml_math.h, operation by operation; x and the result are float32"""
    x = f32(x)
    hi, lo = f32(float.fromhex("0x1.62e42ep6")), f32(float.fromhex("-0x1.9fe368p6"))
    if x != x or np.isinf(x):
        return f32(0.0) if x == -np.inf else x + x
    if x > hi:
        return f32(np.inf)
    if x < lo:
        return f32(0.0)
    xd = float(x)
    inv = float.fromhex("0x1.71547652b82fep+0") * 32.0
    shift = float.fromhex("0x1.8p52")
    c0 = float.fromhex("0x1.c6af84b912394p-5") / 32.0 / 32.0 / 32.0
    c1 = float.fromhex("0x1.ebfce50fac4f3p-3") / 32.0 / 32.0
    c2 = float.fromhex("0x1.62e42ff0c52d6p-1") / 32.0
    z = inv * xd
    kd = z + shift
    ki = _d2u(kd)
    kd = kd - shift
    r = z - kd
    t = (_EXP2F_TAB[ki & 31] + (ki << 47)) & 0xFFFFFFFFFFFFFFFF
    s = _u2d(t)
    z = c0 * r + c1
    r2 = r * r
    y = c2 * r + 1.0
    y = z * r2 + y
    y = y * s
    return f32(y)


def tables(case):
    """(e[B][K] float32 as Python lists, m[B])"""
    K, D, P = case["K"], case["D"], case["P"]
    starts, mv, A = case["starts"], case["mean_var"], case["A"]
    B = len(starts) - 1
    with np.errstate(all="ignore"):
        pmap = [[(s // P ** d) % P for d in range(D)] for s in range(K)]
        logNs, logA = [], []
        for s in range(K):
            r = f32(0.0)
            for d in range(D):
                p = pmap[s][d]
                m, v = f32(mv[2 * p]), f32(mv[2 * p + 1])
                sd = np.sqrt(v)
                r = r + (hml_logf(sd) + (m * m) / (f32(2) * v))
            logNs.append(r)
            logA.append(hml_logf(A[s, s]))
        e_rows, m_out = [], []
        for b in range(B):
            N = f32(int(starts[b + 1]) - int(starts[b]))
            top = f32(-3.40282346638528859812e+38)
            E = []
            for s in range(K):
                r = f32(0.0)
                for d in range(D):
                    p = pmap[s][d]
                    mu, var = float(mv[2 * p]), float(mv[2 * p + 1])
                    sx, sq = float(case["sum"][d, b]), float(case["sum_sq"][d, b])
                    num = 2.0 * mu * sx - sq
                    den = 2.0 * var
                    if den == 0.0:
                        ipd = float("nan") if (num == 0.0 or num != num) else (float("inf") if (num > 0) == (np.copysign(1.0, den) > 0) else float("-inf"))
                    else:
                        ipd = num / den
                    r = r + f32(ipd)
                v = r - N * logNs[s]
                if case["self_trans"]:
                    v = v + (N - f32(1.0)) * logA[s]
                E.append(v)
                top = top if v < top else v
            m_out.append(top)
            e_rows.append([hml_expf(v - top) for v in E])
    return e_rows, m_out


# ---- the recursions, in Python floats ----
def bad(x):
    return not (x > 0.0 and x < math.inf)


def tree_sum(v):
    v = list(v)
    while len(v) > 1:
        w = []
        for i in range(0, len(v), 64):
            s = v[i]
            for x in v[i + 1:i + 64]:
                s = s + x
            w.append(s)
        v = w
    return v[0]


def forward_step(A, e_b, prev, pi=None):
    """(alpha_b, c_b) from alpha_{b-1}; the first block from pi (prev is None)"""
    K = len(e_b)
    a = []
    c = 0.0
    for j in range(K):
        if prev is None:
            v = pi[j] * e_b[j]
        else:
            s = 0.0
            for i in range(K):
                s = s + prev[i] * A[i][j]
            v = e_b[j] * s
        a.append(v)
        c = c + v
    return ([1.0 / K] * K if bad(c) else [v / c for v in a]), c


def backward_step(A, e_next, nxt):
    K = len(e_next)
    v = [e_next[j] * nxt[j] for j in range(K)]
    u = []
    s = 0.0
    for i in range(K):
        t = 0.0
        for j in range(K):
            t = t + A[i][j] * v[j]
        u.append(t)
        s = s + t
    return [1.0 / K] * K if bad(s) else [t / s for t in u]


def smooth(case, e_rows, m):
    """dict(alpha, c, beta, gamma (lists of Python floats), loglik, degenerate, state, run_len, run_state, run_conf)"""
    K = case["K"]
    B = len(e_rows)
    A = [[float(v) for v in row] for row in np.asarray(case["A"], np.float32).reshape(K, K)]
    pi = [float(v) for v in np.asarray(case["pi"], np.float32)]
    e = [[float(v) for v in row] for row in e_rows]
    alpha, c, ell, degenerate = [], [], [], 0
    for b in range(B):
        al, cb = forward_step(A, e[b], alpha[-1] if b else None, pi)
        alpha.append(al)
        c.append(cb)
        degenerate += bad(cb)
        ell.append(float(m[b]) + hml_log(cb))
    beta = [None] * B
    beta[B - 1] = [1.0 / K] * K
    for b in range(B - 2, -1, -1):
        beta[b] = backward_step(A, e[b + 1], beta[b + 1])
    gamma, state = [], []
    for b in range(B):
        g = [alpha[b][i] * beta[b][i] for i in range(K)]
        S = 0.0
        for v in g:
            S = S + v
        row = list(alpha[b]) if bad(S) else [v / S for v in g]
        best = 0
        for i in range(K):
            if row[i] > row[best]:
                best = i
        gamma.append(row)
        state.append(best)
    starts = np.asarray(case["starts"], np.int64)
    run_len, run_state, run_conf = [], [], []
    for b in range(B):
        conf, n = gamma[b][state[b]], int(starts[b + 1] - starts[b])
        if b and run_state[-1] == state[b]:
            run_len[-1] += n
            run_conf[-1] = min(run_conf[-1], conf)
        else:
            run_len.append(n); run_state.append(state[b]); run_conf.append(conf)
    return dict(alpha=alpha, c=c, beta=beta, gamma=gamma, loglik=tree_sum(ell), degenerate=degenerate, state=state, run_len=run_len, run_state=run_state,
                run_conf=run_conf)


def enumerate_paths(case, e_rows, m):
    """all K^B paths: (gamma[B][K], log p(y | theta)) with the path weights in double and every sum by math.fsum"""
    K = case["K"]
    B = len(e_rows)
    A = np.asarray(case["A"], np.float32).reshape(K, K).astype(np.float64)
    pi = np.asarray(case["pi"], np.float32).astype(np.float64)
    per = [[[] for _ in range(K)] for _ in range(B)]
    total = []
    for path in itertools.product(range(K), repeat=B):
        w = float(pi[path[0]])
        for b, s in enumerate(path):
            w *= float(e_rows[b][s])
            if b:
                w *= float(A[path[b - 1], s])
        total.append(w)
        for b, s in enumerate(path):
            per[b][s].append(w)
    Z = math.fsum(total)
    if Z == 0.0:
        return None, -math.inf          # no path has weight
    gamma = [[math.fsum(per[b][s]) / Z for s in range(K)] for b in range(B)]
    return gamma, math.fsum(float(v) for v in m) + math.log(Z)


def stale_from_uniform(case, e_rows, L, W):
    """(forward, backward): the chunks whose entry vector, run from the uniform vector W blocks outside the chunk, differs in a
    word from the sequential recursion's - what a first pass with warm-up W must find stale, at the least for the first of them"""
    K = case["K"]
    B = len(e_rows)
    A = [[float(v) for v in row] for row in np.asarray(case["A"], np.float32).reshape(K, K)]
    e = [[float(v) for v in row] for row in e_rows]
    r = smooth(case, e_rows, [0.0] * B)
    n = (B + L - 1) // L
    fwd, bwd = [], []
    for c in range(1, n):
        lo = c * L
        first = lo - W if lo > W else 0
        if first > 0:
            d = [1.0 / K] * K
            for b in range(first, lo):
                d, _ = forward_step(A, e[b], d)
            if d != r["alpha"][lo - 1]:
                fwd.append(c)
    for c in range(n - 1):
        hi = (c + 1) * L
        cur = hi + W
        if cur < B - 1:
            d = [1.0 / K] * K
            while cur > hi:
                d = backward_step(A, e[cur], d)
                cur -= 1
            if d != r["beta"][hi]:
                bwd.append(c)
    return fwd, bwd


def tool_text(loglik, degenerate, run_len, run_state, run_conf):
    """the `posterior` file: log-likelihood and degenerate count, then the maxsegmentation file's columns plus the confidence"""
    lines = ["%.17g\t%d\n" % (loglik, degenerate)]
    lines += ["%d\t%d\t%.17g\n" % (l, s, c) for l, s, c in zip(run_len, run_state, run_conf)]
    return "".join(lines)

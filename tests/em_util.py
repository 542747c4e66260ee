"""TEST INFRASTRUCTURE: expectation-maximisation over blocks (hml_expected_counts, hml_em_step, hml_em_fit of include/hml.h)
restated in Python floats in the order hammlet_amd/csrc/hml_em_ref.h uses - the E-step behind the smoothing restatement of
tests/posterior_util.py, the M-step, the objective and the fit -, an enumeration of all K^B paths, and the plumbing of the
stand-alone program tests/fixtures/em_ref_main.cpp.  Doubles are compared as their 64-bit words."""
import itertools
import math
import os
import struct
import subprocess

import numpy as np

from tests import posterior_util as pu
from tests.posterior_util import _hex, bad, hml_log, tree_sum, words, words32   # noqa: F401

REPO = pu.REPO
SRC = os.path.join(REPO, "tests", "fixtures", "em_ref_main.cpp")
f32 = np.float32
MAX_STEPS, CONVERGED, DEGENERATE = 0, 1, 2
FLAT = dict(alpha=0.0, beta=0.0, mu0=0.0, nu=0.0, a_off=1.0, a_diag=1.0, pi_alpha=1.0)
PRIOR_KEYS = ("alpha", "beta", "mu0", "nu", "a_off", "a_diag", "pi_alpha")


def build_programs(directory, sanitized=True):
    """the plain build (-Wall -Werror) and, if asked, the sanitizer build of the stand-alone program: name -> path"""
    out = {}
    kinds = [("plain", ["-O2"])]
    if sanitized:
        kinds.append(("sanitized", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]))
    for name, extra in kinds:
        exe = os.path.join(str(directory), "em_" + name)
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off"] + extra + ["-o", exe, SRC], check=True)
        out[name] = exe
    return out


def prior_of(nig4, a_off, a_diag, pi_alpha):
    """the priors as the library widens them: floats, exactly"""
    v = [float(f32(x)) for x in list(nig4) + [a_off, a_diag, pi_alpha]]
    return dict(zip(PRIOR_KEYS, v))


def _dword(x):
    return "%x" % struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def case_text(mode, case, use_prior=False, prior=None, max_steps=0, rel_tol=0.0):
    prior = prior or FLAT
    B = len(case["starts"]) - 1
    head = "%s %d %d %d %d %d %d %d %s" % (mode, case["K"], case["D"], case["P"], 1 if case["self_trans"] else 0, B, 1 if use_prior else 0, max_steps, _dword(rel_tol))
    return "\n".join([head, " ".join(_dword(prior[k]) for k in PRIOR_KEYS), " ".join(map(str, np.asarray(case["starts"]).tolist())), _hex(case["sum"]),
                      _hex(case["sum_sq"]), _hex(case["mean_var"]), _hex(case["A"]), _hex(case["pi"])]) + "\n"


_DOUBLES = ("xi", "first", "stay", "occ", "sx", "sxx", "loglik", "objective", "trace")
_FLOATS = ("mean_var", "A", "pi")


def run_program(exe, mode, case, **kw):
    """the program's words: doubles as uint64 arrays, floats as uint32 arrays, counts as ints"""
    r = subprocess.run([exe], input=case_text(mode, case, **kw), capture_output=True, text=True)
    assert r.stderr == "", r.stderr                     # (the sanitizers report there)
    assert r.returncode == 0, (r.returncode, r.stdout[:200])
    out = {}
    for line in r.stdout.splitlines():
        name, _, rest = line.partition(" ")
        if name in _DOUBLES:
            out[name] = np.array([int(v, 16) for v in rest.split()], np.uint64)
        elif name in _FLOATS:
            out[name] = np.array([int(v, 16) for v in rest.split()], np.uint32)
        elif name == "seconds":
            out[name] = float(rest)
        else:
            out[name] = int(rest)
    return out


# ---- the definition, in Python floats ----
def estep(case):
    """dict(xi[K][K], first, stay, occ, sx[K][D], sxx[K][D], loglik, degenerate, xi_degenerate, gamma)"""
    K, D = case["K"], case["D"]
    e_rows, m = pu.tables(case)
    r = pu.smooth(case, e_rows, m)
    B = len(e_rows)
    A = [[float(v) for v in row] for row in np.asarray(case["A"], np.float32).reshape(K, K)]
    e = [[float(v) for v in row] for row in e_rows]
    starts = [int(v) for v in case["starts"]]
    leaves = [[[] for _ in range(K)] for _ in range(K)]
    xi_degenerate = 0
    for b in range(1, B):
        v = [e[b][j] * r["beta"][b][j] for j in range(K)]
        X = 0.0
        x = [[0.0] * K for _ in range(K)]
        for i in range(K):
            for j in range(K):
                x[i][j] = (r["alpha"][b - 1][i] * A[i][j]) * v[j]
                X = X + x[i][j]
        deg = bad(X)
        xi_degenerate += deg
        for i in range(K):
            for j in range(K):
                leaves[i][j].append(0.0 if deg else x[i][j] / X)
    xi = [[tree_sum(leaves[i][j]) if B > 1 else 0.0 for j in range(K)] for i in range(K)]
    n = [float(starts[b + 1] - starts[b]) for b in range(B)]
    g = r["gamma"]
    sx = [[float(v) for v in row] for row in np.asarray(case["sum"], np.float32).reshape(D, B)]
    sq = [[float(v) for v in row] for row in np.asarray(case["sum_sq"], np.float32).reshape(D, B)]
    occ = [tree_sum([n[b] * g[b][j] for b in range(B)]) for j in range(K)]
    stay = [tree_sum([(n[b] - 1.0) * g[b][j] for b in range(B)]) for j in range(K)]
    s1 = [[tree_sum([g[b][j] * sx[d][b] for b in range(B)]) for d in range(D)] for j in range(K)]
    s2 = [[tree_sum([g[b][j] * sq[d][b] for b in range(B)]) for d in range(D)] for j in range(K)]
    return dict(xi=xi, first=list(g[0]), stay=stay, occ=occ, sx=s1, sxx=s2, loglik=r["loglik"], degenerate=r["degenerate"], xi_degenerate=xi_degenerate,
                gamma=g)


def _div(a, b):
    """IEEE division of Python floats (no exception for a zero divisor)"""
    return float(np.float64(a) / np.float64(b))


def mstep(case, n, use_prior=False, prior=None):
    """(a new case with the M-step's float parameters, kept)"""
    prior = prior or FLAT
    K, D, P = case["K"], case["D"], case["P"]
    mv = np.array(case["mean_var"], np.float32)
    A = np.array(case["A"], np.float32).reshape(K, K)
    pi = np.array(case["pi"], np.float32)
    kept = 0
    with np.errstate(all="ignore"):
        for p in range(P):
            cnt = S = Q = 0.0
            for s in range(K):
                for d in range(D):
                    if (s // P ** d) % P == p:
                        cnt = cnt + n["occ"][s]
                        S = S + n["sx"][s][d]
                        Q = Q + n["sxx"][s][d]
            if bad(cnt):
                kept += 1
                continue
            ss = Q - S * S / cnt
            if ss < 0.0:
                ss = 0.0
            if not use_prior:
                mu, var = S / cnt, ss / cnt
            else:
                dx = S / cnt - prior["mu0"]
                mu = _div(prior["nu"] * prior["mu0"] + S, prior["nu"] + cnt)
                var = _div(prior["beta"] + ss / 2.0 + (cnt * prior["nu"] / (cnt + prior["nu"])) * (dx * dx) / 2.0, prior["alpha"] + cnt / 2.0 + 1.5)
            fm, fv = f32(mu), f32(var)
            if not np.isfinite(fm) or not (fv > 0 and np.isfinite(fv)):
                kept += 1
                continue
            mv[2 * p], mv[2 * p + 1] = fm, fv
        for i in range(K + 1):
            is_pi = i == K
            row, R = [], 0.0
            for j in range(K):
                r = n["first"][j] if is_pi else n["xi"][i][j]
                if not is_pi and i == j and case["self_trans"]:
                    r = r + n["stay"][j]
                if use_prior:
                    r = r + ((prior["pi_alpha"] if is_pi else (prior["a_diag"] if i == j else prior["a_off"])) - 1.0)
                if r < 0.0:
                    r = 0.0
                row.append(r)
                R = R + r
            if bad(R):
                kept += 1
                continue
            for j in range(K):
                if is_pi:
                    pi[j] = f32(row[j] / R)
                else:
                    A[i, j] = f32(row[j] / R)
    return dict(case, mean_var=mv, A=A, pi=pi), kept


def objective(case, loglik, use_prior=False, prior=None):
    if not use_prior:
        return loglik
    prior = prior or FLAT
    K, P = case["K"], case["P"]
    mv, A, pi = case["mean_var"], np.asarray(case["A"]).reshape(K, K), case["pi"]
    t = 0.0
    for p in range(P):
        mu, var = float(mv[2 * p]), float(mv[2 * p + 1])
        dm = mu - prior["mu0"]
        t = t + ((-(prior["alpha"] + 1.5) * hml_log(var) - _div(prior["beta"], var)) - _div(prior["nu"] * (dm * dm), 2.0 * var))
    for i in range(K):
        for j in range(K):
            a1 = (prior["a_diag"] if i == j else prior["a_off"]) - 1.0
            if a1 != 0.0:
                t = t + a1 * hml_log(float(A[i, j]))
    p1 = prior["pi_alpha"] - 1.0
    if p1 != 0.0:
        u = 0.0
        for j in range(K):
            u = u + hml_log(float(pi[j]))
        t = t + p1 * u
    return loglik + t


def fit(case, max_steps, rel_tol=0.0, use_prior=False, prior=None):
    """(the case with the fitted parameters, trace, steps, reason, kept)"""
    trace, kept, k = [], 0, 0
    while True:
        n = estep(case)
        trace.append(objective(case, n["loglik"], use_prior, prior))
        if n["degenerate"] + n["xi_degenerate"] > 0:
            return case, trace, k, DEGENERATE, kept
        if k >= 1 and trace[k] - trace[k - 1] <= rel_tol * abs(trace[k - 1]):
            return case, trace, k, CONVERGED, kept
        if k >= max_steps:
            return case, trace, k, MAX_STEPS, kept
        case, kk = mstep(case, n, use_prior, prior)
        kept += kk
        k += 1


def enumerate_counts(case):
    """all K^B paths (weights in double, sums by math.fsum): dict(xi, first, occ, sx) or None if no path
    has weight"""
    K, D = case["K"], case["D"]
    e_rows, _ = pu.tables(case)
    B = len(e_rows)
    A = np.asarray(case["A"], np.float32).reshape(K, K).astype(np.float64)
    pi = np.asarray(case["pi"], np.float32).astype(np.float64)
    starts = [int(v) for v in case["starts"]]
    sums = np.asarray(case["sum"], np.float32).reshape(D, B).astype(np.float64)
    pair = [[[] for _ in range(K)] for _ in range(K)]
    first = [[] for _ in range(K)]
    occ = [[] for _ in range(K)]
    sx = [[[] for _ in range(D)] for _ in range(K)]
    total = []
    for path in itertools.product(range(K), repeat=B):
        w = float(pi[path[0]])
        for b, s in enumerate(path):
            w *= float(e_rows[b][s])
            if b:
                w *= float(A[path[b - 1], s])
        total.append(w)
        first[path[0]].append(w)
        for b, s in enumerate(path):
            occ[s].append(w * (starts[b + 1] - starts[b]))
            for d in range(D):
                sx[s][d].append(w * float(sums[d, b]))
            if b:
                pair[path[b - 1]][s].append(w)
    Z = math.fsum(total)
    if Z == 0.0:
        return None
    return dict(xi=[[math.fsum(pair[i][j]) / Z for j in range(K)] for i in range(K)], first=[math.fsum(v) / Z for v in first],
                occ=[math.fsum(v) / Z for v in occ], sx=[[math.fsum(sx[j][d]) / Z for d in range(D)] for j in range(K)])


# ---- comparing ----
COUNT_KEYS = ("xi", "first", "stay", "occ", "sx", "sxx")


def same_counts(got, want, what=None):
    """got: words (the program's, or words() of the library's arrays); want: the restatement's Python floats"""
    for key in COUNT_KEYS:
        assert np.array_equal(np.asarray(got[key]).ravel(), words(np.array(want[key], np.float64))), (what, key)
    assert np.asarray(got["loglik"]).ravel()[0] == words([want["loglik"]])[0], what
    assert got["degenerate"] == want["degenerate"] and got["xi_degenerate"] == want["xi_degenerate"], what


def same_parameters(got, case, what=None):
    assert np.array_equal(got["mean_var"], words32(case["mean_var"])), what
    assert np.array_equal(got["A"], words32(case["A"])), what
    assert np.array_equal(got["pi"], words32(case["pi"])), what


def chain_counts_words(n):
    """Chain.expected_counts() as the program prints it"""
    return dict(xi=words(n["xi"]), first=words(n["first"]), stay=words(n["stay"]), occ=words(n["occ"]), sx=words(n["sum"]), sxx=words(n["sum_sq"]),
                loglik=words([n["loglik"]]), degenerate=n["degenerate"], xi_degenerate=n["xi_degenerate"])

"""TEST INFRASTRUCTURE: path sampling under fixed parameters (hml_posterior_sample, hml_posterior_sample_regions of
include/hml.h) restated in Python in the order hammlet_amd/csrc/hml_sample_ref.h uses - the forward rows of
tests/posterior_util.py, Philox4x32-10 in integers, the categorical rule in IEEE doubles (numpy float64, one draw an element:
element-wise +, x and < are the scalar operations) -, an enumeration of all K^B paths, Bernstein's bound, and the plumbing of
the stand-alone program tests/fixtures/sample_ref_main.cpp.  Every output is an integer; they are compared as such."""
import itertools
import math
import os
import subprocess

import numpy as np

from tests import posterior_util as pu
from tests import viterbi_util as vu
from tests.posterior_util import _hex, chain_case, random_case, words   # noqa: F401

REPO = pu.REPO
SRC = os.path.join(REPO, "tests", "fixtures", "sample_ref_main.cpp")
KIND_PSAMPLE = 8
_M32 = np.uint64(0xFFFFFFFF)


def build_programs(directory, sanitized=True):
    """the plain build (-Wall -Werror) and, if asked, the sanitizer build of the stand-alone program: name -> path"""
    out = {}
    kinds = [("plain", ["-O2"])]
    if sanitized:
        kinds.append(("sanitized", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]))
    for name, extra in kinds:
        exe = os.path.join(str(directory), "sample_" + name)
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off"] + extra + ["-o", exe, SRC], check=True)
        out[name] = exe
    return out


def case_text(case, first, count, seed, start=(), end=(), H=8, mode="sample"):
    B = len(case["starts"]) - 1
    head = mode + " %d %d %d %d %d %d %d %d %d %d" % (case["K"], case["D"], case["P"], 1 if case["self_trans"] else 0, B, first, count, seed, len(start), H)
    return "\n".join([head, " ".join(map(str, np.asarray(case["starts"]).tolist())), _hex(case["sum"]), _hex(case["sum_sq"]), _hex(case["mean_var"]),
                      _hex(case["A"]), _hex(case["pi"]), " ".join(map(str, np.asarray(start).tolist())), " ".join(map(str, np.asarray(end).tolist()))]) + "\n"


COUNT_KEYS = ("segments", "score_fixed", "change_count", "state_count", "sample_degenerate")
REGION_KEYS = ("hist", "whole_state", "breaks_sum", "breaks_sq")


def run_program(exe, case, first, count, seed, start=(), end=(), H=8, paths_file=None, mode="sample"):
    """the program's words: dict(paths[count, B] uint8 (if a file is named), segments, score_fixed, change_count, state_count[B, K],
    hist[n, H + 1], whole_state[n, K], breaks_sum, breaks_sq (int64), sample_degenerate, viterbi_score, alpha (uint64 words),
    seconds (before the draws, the draws)); mode "timing": segments, score_fixed, sample_degenerate and seconds alone"""
    r = subprocess.run([exe] + ([paths_file] if paths_file else []), input=case_text(case, first, count, seed, start, end, H, mode), capture_output=True, text=True)
    assert r.stderr == "", r.stderr                     # (the sanitizers report there)
    assert r.returncode == 0, (r.returncode, r.stdout[:200])
    K, B = case["K"], len(case["starts"]) - 1
    out = {}
    for line in r.stdout.splitlines():
        name, _, rest = line.partition(" ")
        if name == "seconds":
            out[name] = [float(v) for v in rest.split()]
        elif name in ("sample_degenerate", "viterbi_score"):
            out[name] = int(rest)
        elif name == "alpha":
            out[name] = np.array([int(v, 16) for v in rest.split()], np.uint64).reshape(B, K)
        else:
            out[name] = np.array(rest.split(), np.int64)
    if mode == "sample":
        out["state_count"] = out["state_count"].reshape(B, K)
        out["hist"] = out["hist"].reshape(-1, H + 1)
        out["whole_state"] = out["whole_state"].reshape(-1, K)
    if paths_file:
        out["paths"] = np.fromfile(paths_file, np.uint8).reshape(count, B)
    return out


def run_pick(exe, w, u):
    """the categorical rule alone, by the program"""
    text = "pick %d %x %s\n" % (len(w), pu._d2u(float(u)), " ".join("%x" % pu._d2u(float(v)) for v in w))
    r = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert r.stderr == "" and r.returncode == 0, (r.stderr, r.stdout)
    return int(r.stdout.split()[1])


# ---- the uniforms ----
def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """uint64 arrays (or scalars) holding 32-bit values"""
    M0, M1, W0, W1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
    c0, c1, c2, c3 = (np.asarray(v, np.uint64) for v in (c0, c1, c2, c3))
    k0, k1 = np.uint64(k0), np.uint64(k1)
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & _M32, (p0 >> s32) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + W0) & _M32, (k1 + W1) & _M32
    return c0, c1, c2, c3


def uniforms(seed, r, b):
    """u of the draws r (uint64 array) at block b, float64"""
    r = np.asarray(r, np.uint64)
    seed = int(seed)
    hi_word = (np.uint64(KIND_PSAMPLE << 24)) | ((r >> np.uint64(32)) & np.uint64(0x00FFFFFF))
    o = philox4x32_10(np.zeros_like(r), np.full_like(r, b >> 1), r & _M32, hi_word, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    hi, lo = (o[2], o[3]) if b & 1 else (o[0], o[1])
    return ((hi >> np.uint64(5)).astype(np.float64) * 67108864.0 + (lo >> np.uint64(6)).astype(np.float64)) * (1.0 / 9007199254740992.0)


# ---- the categorical rule ----
def _bad(S):
    return ~((S > 0.0) & (S < np.inf))


def pick(w, u):
    """(states, S) for weights w[n, K] and uniforms u[n]; where S is bad the state is -1"""
    n, K = w.shape
    c = np.zeros(n)
    cum = np.empty((n, K))
    for i in range(K):
        c = c + w[:, i]
        cum[:, i] = c
    t = u * c
    lt = t[:, None] < cum
    pos = w > 0.0
    last = np.where(pos.any(1), K - 1 - np.argmax(pos[:, ::-1], 1), 0)
    state = np.where(lt.any(1), np.argmax(lt, 1), last)
    return np.where(_bad(c), -1, state), c


def draw_paths(alpha, A, first, count, seed):
    """(paths[count, B] uint8, sample_degenerate) from the rows alpha[B, K] and A[K, K], float64"""
    alpha, A = np.asarray(alpha, np.float64), np.asarray(A, np.float64)
    B, K = alpha.shape
    r = np.arange(first, first + count, dtype=np.uint64)
    q = np.empty((count, B), np.uint8)
    degenerate = 0
    nxt = None
    with np.errstate(all="ignore"):
        for b in range(B - 1, -1, -1):
            u = uniforms(seed, r, b)
            plain = np.broadcast_to(alpha[b], (count, K))
            w = plain if nxt is None else alpha[b][None, :] * A[:, nxt].T
            state, _ = pick(w, u)
            again = state < 0
            if again.any():
                degenerate += int(again.sum())
                s2, _ = pick(plain[again], u[again])
                state[again] = np.where(s2 < 0, 0, s2)
            q[:, b] = state
            nxt = state
    return q, degenerate


# ---- what is read off the paths ----
def block_of(starts, pos):
    return int(np.searchsorted(np.asarray(starts[:-1], np.int64), pos, side="right")) - 1


def path_counts(paths, K, emit=None, trans=None, init=None):
    """dict(segments, score_fixed (if the tables are given), change_count, state_count) of paths[count, B]"""
    paths = np.asarray(paths)
    count, B = paths.shape
    change = paths[:, 1:] != paths[:, :-1]
    out = dict(segments=1 + change.sum(1).astype(np.int64), change_count=np.concatenate([[0], change.sum(0)]).astype(np.int64),
               state_count=np.stack([(paths == j).sum(0) for j in range(K)], 1).astype(np.int64))
    if emit is not None:
        emit, trans, init = np.asarray(emit, np.int64).view(np.uint64), np.asarray(trans, np.int64).view(np.uint64), np.asarray(init, np.int64).view(np.uint64)
        q = paths.astype(np.int64)
        s = init[q[:, 0]].copy()
        s += emit[np.arange(B)[None, :], q].sum(1, dtype=np.uint64)
        if B > 1:
            s += trans[q[:, :-1], q[:, 1:]].sum(1, dtype=np.uint64)
        out["score_fixed"] = s.view(np.int64)
    return out


def region_counts(paths, K, starts, start, end, H):
    """dict(hist[n, H + 1], whole_state[n, K], breaks_sum[n], breaks_sq[n]) recounted from paths[count, B]"""
    paths = np.asarray(paths)
    n = len(start)
    out = dict(hist=np.zeros((n, H + 1), np.int64), whole_state=np.zeros((n, K), np.int64), breaks_sum=np.zeros(n, np.int64), breaks_sq=np.zeros(n, np.int64))
    change = np.concatenate([np.zeros((paths.shape[0], 1), np.int64), np.cumsum(paths[:, 1:] != paths[:, :-1], 1)], 1)
    for g in range(n):
        ba, be = block_of(starts, int(start[g])), block_of(starts, int(end[g]) - 1)
        m = change[:, be] - change[:, ba]
        out["hist"][g] = np.bincount(np.minimum(m, H), minlength=H + 1)
        out["whole_state"][g] = np.bincount(paths[m == 0, ba], minlength=K)
        out["breaks_sum"][g] = m.sum()
        out["breaks_sq"][g] = (m * m).sum()
    return out


def restate(case, first, count, seed, start=(), end=(), H=8):
    """everything the program prints, restated: the forward rows in Python floats, the score tables in Python integers"""
    K = case["K"]
    e_rows, m = pu.tables(case)
    A = [[float(v) for v in row] for row in np.asarray(case["A"], np.float32).reshape(K, K)]
    pi = [float(v) for v in np.asarray(case["pi"], np.float32)]
    alpha = []
    for b, e in enumerate(e_rows):
        alpha.append(pu.forward_step(A, [float(v) for v in e], alpha[-1] if b else None, pi)[0])
    emit, trans, init = vu.tables(case)
    paths, degenerate = draw_paths(alpha, A, first, count, seed)
    wrap = lambda rows: np.array([[vu.wrap64(v) for v in row] for row in rows], np.int64)
    out = path_counts(paths, K, wrap(emit), wrap(trans), wrap([init])[0])
    out.update(region_counts(paths, K, case["starts"], start, end, H))
    _, vscore, _, _ = vu.decode(emit, trans, init)
    out.update(paths=paths, sample_degenerate=degenerate, viterbi_score=vscore, alpha=words(np.array(alpha, np.float64)).reshape(-1, K))
    return out


def same(got, want, keys, what=None):
    for key in keys:
        assert np.array_equal(np.asarray(got[key]).astype(np.int64), np.asarray(want[key]).astype(np.int64)), (what, key)


def invariants(r, K, count, viterbi_score, A=None, pi=None):
    """what holds for every sample: r has paths, segments, score_fixed, change_count, state_count"""
    assert np.all(np.asarray(r["score_fixed"], np.int64) <= viterbi_score)
    assert int(np.asarray(r["change_count"], np.int64).sum()) == int((np.asarray(r["segments"], np.int64) - 1).sum())
    assert np.all(np.asarray(r["state_count"], np.int64).sum(1) == count)
    paths = np.asarray(r["paths"])
    assert paths.max() < K
    if A is not None:
        A = np.asarray(A).reshape(K, K)
        assert np.all(np.asarray(pi)[paths[:, 0]] > 0)
        if paths.shape[1] > 1:
            assert np.all(A[paths[:, :-1], paths[:, 1:]] > 0)


# ---- all paths, and Bernstein's bound ----
def path_probabilities(case):
    """p[K^B] of every path, indexed by sum_b q_b K^b; None if no path has weight"""
    K = case["K"]
    e_rows, _ = pu.tables(case)
    B = len(e_rows)
    A = np.asarray(case["A"], np.float32).reshape(K, K).astype(np.float64)
    pi = np.asarray(case["pi"], np.float32).astype(np.float64)
    w = np.zeros(K ** B)
    for path in itertools.product(range(K), repeat=B):
        v = float(pi[path[0]])
        for b, s in enumerate(path):
            v *= float(e_rows[b][s])
            if b:
                v *= float(A[path[b - 1], s])
        w[sum(s * K ** b for b, s in enumerate(path))] = v
    Z = math.fsum(w)
    return None if Z == 0.0 else w / Z


def bernstein(R, p, delta=1e-12):
    """the deviation |count - R p| of a binomial(R, p) count that has probability at most delta"""
    lam = math.log(2.0 / delta)
    v = R * p * (1.0 - p)
    return lam / 3.0 + np.sqrt(lam * lam / 9.0 + 2.0 * v * lam)

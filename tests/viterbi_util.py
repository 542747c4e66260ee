"""TEST INFRASTRUCTURE: the Viterbi decode of include/hml.h (hml_viterbi) restated in Python - the tables with numpy float32 /
Python float (IEEE double) arithmetic in the order hammlet_amd/csrc/hml_viterbi_ref.h uses, the recursion, the back-track, the
score and a brute-force search in Python integers - and the plumbing of the stand-alone program tests/fixtures/viterbi_ref_main.cpp.
"""
import itertools
import os
import struct
import subprocess

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "fixtures", "viterbi_ref_main.cpp")
LIM = 2 ** 38
ONE = 2 ** 20
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


def _bits(a):
    return np.ascontiguousarray(a, np.float32).ravel().view(np.uint32)


def _hex(a):
    return " ".join(map("%x".__mod__, _bits(a).tolist()))


def case_text(case, want_emit=True):
    """a case - dict(K, D, P, self_trans, starts, sum[D, B], sum_sq[D, B], mean_var[2 P], A[K, K], pi[K]) - as the program reads it"""
    B = len(case["starts"]) - 1
    head = "case %d %d %d %d %d %d" % (case["K"], case["D"], case["P"], 1 if case["self_trans"] else 0, B, 1 if want_emit else 0)
    return "\n".join([head, " ".join(map(str, np.asarray(case["starts"]).tolist())), _hex(case["sum"]), _hex(case["sum_sq"]), _hex(case["mean_var"]),
                      _hex(case["A"]), _hex(case["pi"])]) + "\n"


def run_program(exe, text):
    r = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert r.stderr == "", r.stderr                     # (the sanitizers report there)
    assert r.returncode == 0, (r.returncode, r.stdout[:200])
    out = {}
    for line in r.stdout.splitlines():
        name, _, rest = line.partition(" ")
        if name == "seconds":
            out[name] = [float(v) for v in rest.split()]
        else:
            out[name] = np.array(rest.split(), np.int64) if name != "score" else int(rest)
    return out


def run_case(exe, case, want_emit=True):
    """dict(init[K], trans[K, K], emit[B, K] (if asked), path[B], score) from the program"""
    out = run_program(exe, case_text(case, want_emit))
    K = case["K"]
    out["trans"] = out["trans"].reshape(K, K)
    if want_emit:
        out["emit"] = out["emit"].reshape(-1, K)
    return out


def run_fx(exe, values):
    return run_program(exe, "fx %d\n%s\n" % (len(values), _hex(values)))["fx"]


def make_case(K, starts, sum_x, sum_xx, mean_var, A, pi, D=1, P=None, self_trans=True):
    B = len(starts) - 1
    return dict(K=K, D=D, P=P or K, self_trans=self_trans, starts=np.asarray(starts, np.uint32),
                sum=np.asarray(sum_x, np.float32).reshape(D, B), sum_sq=np.asarray(sum_xx, np.float32).reshape(D, B),
                mean_var=np.asarray(mean_var, np.float32), A=np.asarray(A, np.float32).reshape(K, K), pi=np.asarray(pi, np.float32))


def chain_case(g, self_trans=True):
    """the case of a chain's current blocks and parameters, from the GPU's own read-outs"""
    A, pi = g.transitions()
    sx, sq = g.block_stats()
    return make_case(g.K, g.blocks(), sx, sq, g.theta(), A, pi, D=g.D, P=g.P or g.K, self_trans=self_trans)


# ---- the tables ----
def fx(x):
    """llrint(clamp(x, -2^38, 2^38) 2^20), not-a-number as -2^38; x a float (exactly a double)"""
    x = float(x)
    if x != x:
        x = -float(LIM)
    x = min(max(x, -float(LIM)), float(LIM))
    y = x * float(ONE)                    # exact
    r = int(y)                            # toward zero; exact for |y| >= 2^53 (already whole)
    d = y - r                             # exact
    if abs(d) > 0.5 or (abs(d) == 0.5 and r % 2 != 0):
        r += 1 if d > 0 else -1
    return r


def _d2u(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def _u2d(u):
    return struct.unpack("<d", struct.pack("<Q", u))[0]


def hml_log(x):
    """hml_log of hammlet_amd/csrc/hml_math.h, operation by operation (Python floats are IEEE doubles)"""
    ln2_hi, ln2_lo = 6.93147180369123816490e-01, 1.90821492927058770002e-10
    Lg1, Lg2, Lg3, Lg4 = 6.666666666666735130e-01, 3.999999999940941908e-01, 2.857142874366239149e-01, 2.222219843214978396e-01
    Lg5, Lg6, Lg7 = 1.818357216161805012e-01, 1.531383769920937332e-01, 1.479819860511658591e-01
    ux = _d2u(x)
    if (ux << 1) & 0xFFFFFFFFFFFFFFFF == 0:
        return float("-inf")
    if ux >> 63:
        return float("nan")
    if (ux >> 52) >= 0x7FF:
        return x
    k = 0
    if (ux >> 52) == 0:
        x = x * 18014398509481984.0
        ux = _d2u(x)
        k = -54
    hx = (ux >> 32) & 0xFFFFFFFF
    hx = (hx + 0x3FF00000 - 0x3FE6A09E) & 0xFFFFFFFF
    k += (hx >> 20) - 0x3FF
    hx = (hx & 0x000FFFFF) + 0x3FE6A09E
    ux = (hx << 32) | (ux & 0xFFFFFFFF)
    m = _u2d(ux)
    f = m - 1.0
    hfsq = 0.5 * f * f
    s = f / (2.0 + f)
    z = s * s
    w = z * z
    t1 = w * (Lg2 + w * (Lg4 + w * Lg6))
    t2 = z * (Lg1 + w * (Lg3 + w * (Lg5 + w * Lg7)))
    R = t2 + t1
    dk = float(k)
    return dk * ln2_hi - ((hfsq - (s * (hfsq + R) + dk * ln2_lo)) - f)


def hml_logf(x):
    return f32(hml_log(float(f32(x))))


def tables(case):
    """(emit[B][K], trans[K][K], init[K]) as lists of Python integers"""
    K, D, P = case["K"], case["D"], case["P"]
    starts, mv, A, pi = case["starts"], case["mean_var"], case["A"], case["pi"]
    B = len(starts) - 1
    with np.errstate(all="ignore"):
        init = [fx(hml_logf(pi[j])) for j in range(K)]
        trans = [[fx(hml_logf(A[i, j])) for j in range(K)] for i in range(K)]
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
        emit = []
        for b in range(B):
            N = f32(int(starts[b + 1]) - int(starts[b]))
            row = []
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
                e = r - N * logNs[s]
                if case["self_trans"]:
                    e = e + (N - f32(1.0)) * logA[s]
                row.append(fx(e))
            emit.append(row)
    return emit, trans, init


# ---- the recursion ----
def step(d, trans, emit_b):
    """one block: (normalised vector, back-pointers), the smallest index among equal maxima"""
    K = len(d)
    nd, psi = [], []
    for j in range(K):
        best, arg = d[0] + trans[0][j], 0
        for i in range(1, K):
            v = d[i] + trans[i][j]
            if v > best:
                best, arg = v, i
        nd.append(best + emit_b[j])
        psi.append(arg)
    top = max(nd)
    return [v - top for v in nd], psi


def first_vector(emit, init):
    d = [init[j] + emit[0][j] for j in range(len(init))]
    top = max(d)
    return [v - top for v in d]


def wrap64(v):
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >= (1 << 63) else v


def path_score(path, emit, trans, init):
    s = init[path[0]]
    for b, q in enumerate(path):
        s += emit[b][q]
        if b:
            s += trans[path[b - 1]][q]
    return s


def decode(emit, trans, init):
    """(path, score wrapped to int64, psi rows, the normalised vector after every block)"""
    B = len(emit)
    d = first_vector(emit, init)
    psis, vecs = [None], [d]
    for b in range(1, B):
        d, psi = step(d, trans, emit[b])
        psis.append(psi)
        vecs.append(d)
    s = d.index(0)
    path = [0] * B
    for b in range(B - 1, -1, -1):
        path[b] = s
        if b:
            s = psis[b][s]
    return path, wrap64(path_score(path, emit, trans, init)), psis, vecs


def brute_force(emit, trans, init):
    """all K^B paths in Python integers: (the maximal score, the maximal path that is smallest read from the LAST block backwards)"""
    B, K = len(emit), len(init)
    best, arg = None, None
    for path in itertools.product(range(K), repeat=B):
        s = path_score(path, emit, trans, init)
        key = tuple(reversed(path))
        if best is None or s > best or (s == best and key < arg):
            best, arg = s, key
    return best, list(reversed(arg))


def stale_chunks_from_zero(emit, trans, init, L, W):
    """the chunks c >= 1 whose vector at block c L - 1, run from the zero vector W blocks early (from `init` where that reaches
    block 0), differs from the sequential recursion's there: what a first pass with warm-up W must find stale, at the least
    for the first of them"""
    B, K = len(emit), len(init)
    vecs = decode(emit, trans, init)[3]
    stale = []
    for c in range(1, (B + L - 1) // L):
        lo = c * L
        first = lo - W if lo > W else 0
        if first == 0:
            continue
        d = [0] * K
        for b in range(first, lo):
            d, _ = step(d, trans, emit[b])
        if d != vecs[lo - 1]:
            stale.append(c)
    return stale


def runs_of(path, starts):
    """(run_len, run_state): adjacent blocks of equal state merged, lengths in positions"""
    path = np.asarray(path)
    starts = np.asarray(starts, np.int64)
    first = np.flatnonzero(np.concatenate([[True], path[1:] != path[:-1]]))
    bounds = np.concatenate([starts[first], [starts[-1]]])
    return np.diff(bounds).astype(np.uint64), path[first].astype(np.int32)


def tool_text(run_len, run_state):
    """the `maxsegmentation` file's format (the tool's running state starts at 0)"""
    lines = []
    if len(run_state) and run_state[0] != 0:
        lines.append("0\t0\n")
    lines += ["%d\t%d\n" % (l, s) for l, s in zip(run_len, run_state)]
    return "".join(lines)

"""TEST INFRASTRUCTURE: planted cases for the exact-inference passes (hml_infer.hip) at hostile magnitudes, in the make_case
format of tests/viterbi_util.py - data from ol.trace, ol.synth_depth and integer arithmetic alone, statistics summed on the host
("ideal": a chain's own come out of its integral array and differ in the last bits), parameters planted by hand - and the
coverage flags that say which data-dependent mechanism a case reaches.

CASES: name -> function(T=None) returning the recipe dict(x, K, D, P, self_trans, block, mean_var, A, pi): `block` positions a
block (1: every position a block).  EXPECT: name -> the flags the case is in the table for.  DEVICE: the names a chain can be
put on: data loaded, every position a block, set_parameters.  Not on the device: ten blocks of 5000 positions (50 000 positions;
the hostile chains of tests/test_gpu_infer_hostile.py form such blocks by themselves) and `overflow`, whose sum of squares is
infinite - a chain's integral array then holds inf - inf behind the first position, which is another case."""
import numpy as np

from tests import oracle_lib as ol
from tests import viterbi_util as vu
from tests.hostile_inputs import _hash

f32 = np.float32
DENORMAL = f32(2.0 ** -149)
T_DEFAULT = 80          # at least 65 blocks: 64 clamped emission scores wrap the 64-bit path score
FLAGS = ("all_degenerate", "partly_degenerate", "loglik_minus_inf", "loglik_nan", "denormal_e", "clamped_and_wrapped", "xi_degenerate",
         "pair_degenerate", "sample_degenerate", "em_degenerate", "mstep_bad_variance", "ip_close", "ip_product_differs", "ip_tiny", "ip_huge", "ip_not_finite", "ip_common")


def sticky(K, stay=0.9):
    A = np.full((K, K), (1.0 - stay) / (K - 1), f32)
    np.fill_diagonal(A, stay)
    return A


def levels(K):
    return np.array(ol.LEVELS[K] if K in ol.LEVELS else np.arange(K) - (K - 1) / 2.0, f32)


def mean_var(mu, var):
    mu = np.asarray(mu, f32)
    return np.stack([mu, np.broadcast_to(np.asarray(var, f32), mu.shape)], 1).ravel().astype(f32)


def follow(x, K):
    """parameters that follow data of any kind: means at K quantiles of the sorted data, one variance - a K-th of the data's,
    rounded to sixteenths so that the last bit of a floating-point variance does not matter; wide enough that every state keeps
    some weight in a fit (a state without any gets A_ss = 0, and 0 x -inf in the next E-step is a NaN whose sign the host's
    compiler chooses when it meets log(NaN) in a sum - tests/test_gpu_posterior.py)"""
    s = np.sort(np.asarray(x, np.float64))
    mu = s[[(2 * k + 1) * s.size // (2 * K) for k in range(K)]]
    var = np.round(s.var() / K * 16.0) / 16.0 + 0.0625
    return mean_var(mu, var)


def uniform(K):
    return np.full(K, 1.0 / K, f32)


def switching(T, K, seed):
    """every 500th position of ol.trace: the level changes every few positions instead of every few thousand"""
    return np.ascontiguousarray(ol.trace(500 * T, K, seed)[::500])


CASES, EXPECT, DEVICE = {}, {}, []


def _add(name, fn, expect=(), device=True):
    assert set(expect) <= set(FLAGS), expect
    CASES[name] = fn
    EXPECT[name] = frozenset(expect)
    if device:
        DEVICE.append(name)


def _recipe(x, K, mv, A=None, pi=None, D=1, P=None, self_trans=True, block=1):
    return dict(x=np.ascontiguousarray(x, f32), K=K, D=D, P=P or K, self_trans=self_trans, block=block, mean_var=np.asarray(mv, f32),
                A=sticky(K) if A is None else np.asarray(A, f32), pi=uniform(K) if pi is None else np.asarray(pi, f32))


def _scaled(k, following):
    def fn(T=None):
        x = np.ldexp(switching(T or T_DEFAULT, 3, 1), k).astype(f32)
        mv = mean_var(np.ldexp(levels(3), k), np.ldexp(f32(0.04), 2 * k)) if following else mean_var(levels(3), 0.04)
        return _recipe(x, 3, mv)
    return fn


for _k in (10, 40, -10, -40):
    _n = "scale_2%s%d" % ("m" if _k < 0 else "p", abs(_k))
    _add(_n + "_follow", _scaled(_k, True), ["ip_common"])
    # every E of 2^40-scaled data under unit-scale parameters is below -2^38: every emission score clamps, all states tie
    _add(_n + "_unit", _scaled(_k, False), ["clamped_and_wrapped"] if _k == 40 else [])


def _offset(c, K):
    return lambda T=None: _recipe((switching(T or T_DEFAULT, K, 2) + f32(c)).astype(f32), K, mean_var(levels(K) + f32(c), 0.04))


_add("offset_100_k5", _offset(100, 5))
_add("offset_1000_k2", _offset(1000, 2))


def _sticky5000(T=None):
    """ten blocks of 5000 positions; states 1 and 2 are twins in the emission and differ on the diagonal of A by a factor of
    exp(-0.019): 4999 log A_22 - 4999 log A_11 = -95, and e_b(2) is a float denormal wherever a twin is on top"""
    A = np.array([[0.99, 0.005, 0.005], [0.005, 0.99, 0.005], [0.014, 0.0146, 0.9714]], f32)
    return _recipe(ol.trace(T or 50000, 3, 1), 3, mean_var([-5.0, 0.0, 0.0], 1.0), A=A, block=5000)


_add("sticky_5000", _sticky5000, ["denormal_e"], device=False)


def _depth(depth, K, seed):
    def fn(T=None):
        x = ol.synth_depth(T or T_DEFAULT, depth=depth, seed=seed)
        return _recipe(x, K, follow(x, K))
    return fn


_add("depth1_k3", _depth(1.0, 3, 3))
_add("depth5000_k5", _depth(5000.0, 5, 4))


def _k20(T=None):
    """twenty levels a unit apart in runs of four positions, 2^10-scaled, parameters that follow the scale"""
    T = T or T_DEFAULT
    level = (_hash(T // 4 + 1, 9) % 20).repeat(4)[:T].astype(f32) - f32(9.5)
    x = np.ldexp(level + f32(0.125) * switching(T, 3, 4), 10).astype(f32)
    return _recipe(x, 20, mean_var(np.ldexp(levels(20), 10), np.ldexp(f32(0.04), 20)))


_add("k20_scale_2p10", _k20)


def _var_denormal(T=None):
    """state 0 has the smallest variance that can be planted: its inner product is +-inf as a float and its log-normaliser +inf, so
    E_0 is inf - inf = NaN where the position lies in (-2, 0) - around state 0's own level - and -inf elsewhere"""
    mv = mean_var(levels(3), 0.04)
    mv[1] = DENORMAL
    return _recipe(switching(T or T_DEFAULT, 3, 3), 3, mv)


_add("var_denormal", _var_denormal, ["partly_degenerate", "loglik_nan", "xi_degenerate", "pair_degenerate", "em_degenerate", "ip_huge"])


def _nan_before_minus_inf(T=None):
    """every variance the smallest denormal, means -1, 0, 0: at a position in (-2, 0) E is (NaN, -inf, -inf), elsewhere all -inf.
    The running maximum `(v < top) ? top : v` takes the NaN and then leaves it for -inf: m_b = -inf and every e_b is
    expf(-inf + inf) or expf(NaN) - where a maximum instruction, which skips a NaN, keeps -FLT_MAX and finds e_b = 0.
    (A NaN in the LAST state stays in m_b; then m_b + log(c_b) adds the NaN the processor made to the NaN hml_log returns for
    it, two different words on the host, and which of them a sum returns is its compiler's choice: no case for a host test.)"""
    return _recipe(switching(T or T_DEFAULT, 3, 3), 3, mean_var([-1.0, 0.0, 0.0], DENORMAL))


_add("nan_before_minus_inf", _nan_before_minus_inf, ["all_degenerate", "loglik_nan", "ip_huge"])


def _all_degenerate(T=None):
    """data between 2 and 6, every mean 0 and every variance the smallest denormal: every inner product -x^2 2^147 is -inf as a
    float, every E is -inf, every e is 0, every block is reset"""
    x = (switching(T or T_DEFAULT, 3, 1) + f32(4.0)).astype(f32)
    return _recipe(x, 3, mean_var(np.zeros(3), DENORMAL))


_add("all_degenerate", _all_degenerate, ["all_degenerate", "loglik_minus_inf", "xi_degenerate", "pair_degenerate", "em_degenerate", "ip_huge"])


def _small_variance(T=None):
    """unit-scale data, variances of 0.005: the neighbouring level lies 14 sigma away, exp(-100) - a float denormal"""
    return _recipe(switching(T or T_DEFAULT, 3, 1), 3, mean_var(levels(3), 0.005))


_add("small_variance", _small_variance, ["denormal_e"])


def _unreachable(T=None):
    """tests/test_gpu_posterior.py's block no path reaches, at an offset of 1000: pi is all on one state, that state leads to one
    state alone, and position 1 lies 50 sigma and more from that state's level (self-transitions off, as there)"""
    x = (switching(T or T_DEFAULT, 3, 2) + f32(1000.0)).astype(f32)
    mu = levels(3) + f32(1000.0)
    far = int(np.argmax(np.abs(x[1] - mu)))
    first = (far + 1) % 3
    A = np.full((3, 3), 0.25, f32)
    np.fill_diagonal(A, 0.5)
    A[first] = 0.0
    A[first, far] = 1.0
    pi = np.zeros(3, f32)
    pi[first] = 1.0
    return _recipe(x, 3, mean_var(mu, 0.0004), A=A, pi=pi, self_trans=False)


_add("unreachable_offset_1000", _unreachable, ["partly_degenerate", "loglik_minus_inf", "sample_degenerate", "xi_degenerate", "pair_degenerate", "em_degenerate"])


TIE_MEAN, TIE_VAR, TIE_X = 1785.1995849609375, 389 * 2.0 ** -13, 1801.0


def _midpoint(T=None):
    """Small integers and three positions of 1801: a chain's statistics of them are exact (the squares sum to less than 2^24).
    State 0: at x = 1801 = (2^25 - 1) / 18631 the numerator x (2 mu - x) is (2^25 - 1) x 2 var exactly, so the inner product is
    2^25 - 1, the midpoint of the floats 2^25 - 2 and 2^25: the quotient is exact and rounds to even, 2^25; the product with the
    double reciprocal of 2 var = 389 x 2^-12, which is 1.3 x 2^-54 too small, is one double below the midpoint and rounds to
    2^25 - 2.  With float statistics, means and variances the product can differ from the quotient in no other way: a quotient
    that is not a midpoint lies 2^-49 of its value or more from the next one, the product within 2^-52.  E_0 is about -2600
    there, so the 2 shows in m_b and in the decode's score.  State 1: mean 2^-26, variance 0.5, for which 2 mu - 1 at x = 1 is
    the midpoint -(1 - 2^-25), product and quotient alike."""
    T = T or T_DEFAULT
    x = (_hash(T, 5) % 4).astype(f32)
    x[[T // 8, T // 2, 3 * T // 4]] = TIE_X
    return _recipe(x, 2, np.array([TIE_MEAN, TIE_VAR, 2.0 ** -26, 0.5], f32))


_add("midpoint_k2", _midpoint, ["ip_close", "ip_product_differs", "ip_common"])


def _tiny(T=None):
    """2^-40-scaled data; state 1 has mean 0 and variance 2^40: its inner product -x^2 / 2^41 is about 2^-121"""
    mv = mean_var(levels(3), 0.04)
    mv[3] = f32(2.0 ** 40)
    return _recipe(np.ldexp(switching(T or T_DEFAULT, 3, 1), -40).astype(f32), 3, mv)


_add("ip_tiny", _tiny, ["ip_tiny"])


def _overflow(T=None):
    """2^70-scaled data: the squares overflow to inf, every inner product is -inf in double already"""
    return _recipe(np.ldexp(switching(T or T_DEFAULT, 3, 1), 70).astype(f32), 3, mean_var(levels(3), 0.04))


_add("overflow", _overflow, ["ip_not_finite", "all_degenerate"], device=False)


def _plateaus(T=None):
    """plateaus of ten equal integers and variances of 0.0004: every gamma is exactly 0 or 1, so the M-step's sum of squares
    cancels to exactly 0 and the variance it yields is 0 - kept out of the model"""
    x = ((np.arange(T or T_DEFAULT) // 10) % 2).astype(f32)
    return _recipe(x, 2, mean_var([0.0, 1.0], 0.0004))


_add("plateaus_exact", _plateaus, ["mstep_bad_variance"])


def _d2p2(T=None):
    """two data dimensions over two parameters, four states, 2^10-scaled with parameters that follow"""
    T = T or T_DEFAULT
    x = np.ldexp(np.stack([switching(T, 3, 1), switching(T, 3, 2)], axis=1), 10).astype(f32).reshape(-1)
    return _recipe(x, 4, mean_var(np.ldexp(f32([-1.0, 1.0]), 10), np.ldexp(f32(0.25), 20)), D=2, P=2)


_add("d2p2_scale_2p10", _d2p2)


# ---------------------------------------------------------------------------------------------- the case of a recipe
def ideal_case(r):
    """make_case of the recipe with the statistics summed on the host in float"""
    D = r["D"]
    x = r["x"].reshape(-1, D)
    T = x.shape[0]
    starts = np.append(np.arange(0, T, r["block"]), T)
    sq = x * x
    sx = np.stack([[x[a:e, d].sum(dtype=f32) for a, e in zip(starts[:-1], starts[1:])] for d in range(D)])
    sxx = np.stack([[sq[a:e, d].sum(dtype=f32) for a, e in zip(starts[:-1], starts[1:])] for d in range(D)])
    return vu.make_case(r["K"], starts, sx, sxx, r["mean_var"], r["A"], r["pi"], D=D, P=r["P"], self_trans=r["self_trans"])


def case(name, T=None):
    with np.errstate(all="ignore"):
        return ideal_case(CASES[name](T))


# ---------------------------------------------------------------------------------------------- the flags
def ip_grounds(c):
    """hml_inner_product's branch test (hml_k_forward.h) restated on the case's statistics and parameters: the set of
    "ip_common", "ip_close", "ip_tiny", "ip_huge", "ip_not_finite" over every block, state and dimension - and
    "ip_product_differs" where the division it takes yields another float than the product would have"""
    K, D, P = c["K"], c["D"], c["P"]
    out = set()
    with np.errstate(all="ignore"):
        for p in range(P):
            mu, var = np.float64(c["mean_var"][2 * p]), np.float64(c["mean_var"][2 * p + 1])
            rvar = np.float64(1.0) / (np.float64(2.0) * var)
            num = 2.0 * mu * c["sum"].astype(np.float64).ravel() - c["sum_sq"].astype(np.float64).ravel()
            ipd = num * rvar
            bits = ipd.view(np.uint64)
            low = (bits & np.uint64(0x1FFFFFFF)).astype(np.int64)
            ex = ((bits >> np.uint64(52)) & np.uint64(0x7FF)).astype(np.int64)
            close = ((low - 0x0FFFFFFC) & 0xFFFFFFFF) <= 8
            outside = close | (ex < 923) | (ex > 1150)
            divides = outside & ((ipd != 0.0) | close)
            if np.any(~divides):
                out.add("ip_common")
            if np.any(divides & close & (ex >= 923) & (ex <= 1150)):
                out.add("ip_close")
            if np.any(divides & (ex < 923)):
                out.add("ip_tiny")
            if np.any(divides & (ex > 1150) & (ex < 0x7FF)):
                out.add("ip_huge")
            if np.any(divides & (ex == 0x7FF)):
                out.add("ip_not_finite")
            q = (num / (np.float64(2.0) * var)).astype(f32)
            if np.any(divides & (q == q) & (ipd.astype(f32) != q)):
                out.add("ip_product_differs")
    return out


def bad_variance(c, occ, sx, sxx):
    """the maximum-likelihood M-step's variance of some parameter (hml_em_ref.h; tests/em_util.mstep) is not a positive finite
    float although its count is good; occ[K], sx[K][D], sxx[K][D] in doubles"""
    K, D, P = c["K"], c["D"], c["P"]
    with np.errstate(all="ignore"):
        for p in range(P):
            cnt = S = Q = 0.0
            for s in range(K):
                for d in range(D):
                    if (s // P ** d) % P == p:
                        cnt, S, Q = cnt + float(occ[s]), S + float(sx[s][d]), Q + float(sxx[s][d])
            if not (cnt > 0.0 and cnt < np.inf):
                continue
            ss = Q - S * S / cnt
            fv = f32(max(ss, 0.0) / cnt) if ss == ss else f32(np.nan)
            if not (fv > 0 and np.isfinite(fv)):
                return True
    return False


def flags(c, r):
    """the flags of a case from the results of the passes on it: r = dict(degenerate, loglik, e[B, K] float32, emit[B, K] (integers),
    score_plain (the path's score before it wraps), score, xi_degenerate, pair_degenerate, sample_degenerate, reasons (of the fits), occ, sx,
    sxx)"""
    B = len(c["starts"]) - 1
    out = ip_grounds(c)
    if r["degenerate"] == B:
        out.add("all_degenerate")
    if 0 < r["degenerate"] < B:
        out.add("partly_degenerate")
    if r["loglik"] == -np.inf:
        out.add("loglik_minus_inf")
    if r["loglik"] != r["loglik"]:
        out.add("loglik_nan")
    e = np.asarray(r["e"], f32)
    if np.any((e > 0) & (e < f32(2.0 ** -126))):
        out.add("denormal_e")
    if np.all(np.abs(np.asarray(r["emit"], np.int64)) == vu.LIM * vu.ONE) and r["score_plain"] != r["score"]:
        out.add("clamped_and_wrapped")
    for key in ("xi_degenerate", "pair_degenerate", "sample_degenerate"):
        if r[key] > 0:
            out.add(key)
    if 2 in r["reasons"]:          # HML_EM_DEGENERATE
        out.add("em_degenerate")
    if r["degenerate"] + r["xi_degenerate"] == 0 and bad_variance(c, r["occ"], r["sx"], r["sxx"]):
        out.add("mstep_bad_variance")
    return out

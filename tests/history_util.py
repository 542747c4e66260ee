"""TEST INFRASTRUCTURE: the chain's history (include/hml.h, hml_set_history ... hml_history_summary) restated in numpy.

expected(case): the CPU CHECKER stepped through the case's scheme one sweep per call; after every sweep its counts, theta, A,
pi, first state, number of blocks and the threshold of its theta give the row of include/hml.h's table, evaluated in float64 (math.fsum over the
addends: the reference's own rounding is one ulp of the result).  Nothing here comes from the product.

The bound of columns 2-5: (number of addends + 16) 2^-52 sum |addend|.  Every addend - n_p/2 log(2 pi var_p), Sxx_p / (2 var_p),
2 mu_p Sx_p / (2 var_p), n_p mu_p^2 / (2 var_p), N_ij log A_ij, ... - is a product of exactly widened floats and integers after at
most sixteen double roundings, the device's log among them (counted generously), so it is off by at most 16 2^-53 of itself
however the product groups its operations; a sum of t addends in any order adds at most t 2^-53 sum |addend|.

stats(x): hml_history_stats restated (split R-hat, Geyer's initial monotone sequence), for tests/test_history_stats_cpu.py and
the summary test."""
import math

import numpy as np

from tests import oracle_lib as ol

COLS = ("sweep", "method", "ll_emit", "ll_path", "lprior_theta", "lprior_path", "segments", "blocks", "states_used", "threshold", "chain")
EXACT = (0, 1, 6, 7, 8, 9, 10)
BOUNDED = (2, 3, 4, 5)
DIRICHLET = dict(a_off=0.5, a_diag=0.5, pi_alpha=0.5)      # the defaults of the checker and of Chain.set_model
U = 2.0 ** -52


def checker(case, chain=0, seed=None):
    """the checker of a case (tests/breaks_cases.checker) and the prior it was given: (chain, nig4 float32)"""
    mode = (ol.RNG_MT, ol.MATH_LIBM, ol.REDUCE_REF) if case["compat"] else (ol.RNG_CTR, ol.MATH_DEV, ol.REDUCE_DEV)
    o = ol.OracleChain(K=case["K"], seed=case["seed"] if seed is None else seed, chain=chain, rng=mode[0], math=mode[1], reduce=mode[2],
                       weight_mult=case.get("weight_mult", 1.0))
    if case["D"] > 1:
        o.set_dimensions(case["D"], case["P"])
    o.load(case["trace"]() if callable(case["trace"]) else case["trace"])
    prior = o.autoprior().copy()
    o.init_model()
    return o, prior


def _total(addends):
    """(sum of the addends as IEEE gives it - exactly rounded when all are finite -, the bound of a double sum of them)"""
    a = np.asarray(addends, np.float64).reshape(-1)
    if np.all(np.isfinite(a)):
        return math.fsum(a), (len(a) + 16) * U * float(np.sum(np.abs(a)))
    with np.errstate(invalid="ignore"):
        return float(np.sum(a)), float("nan")


def _times(coef, logs):
    """coef * log with the rule of include/hml.h: a product whose count or coefficient is 0 is 0, whatever the logarithm"""
    coef = np.asarray(coef, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(coef == 0, 0.0, coef * np.where(coef == 0, 0.0, logs))


def terms_per_parameter(occ, K, D, P):
    """n_p: the (position, dimension) terms of parameter p - n(p) for D = 1, sum_s n(s) #{d: map[s][d] = p} with map[s][d] = (s / P^d) % P"""
    if D == 1:
        return np.asarray(occ, np.uint64).copy()
    n = np.zeros(P, np.uint64)
    for s in range(K):
        for d in range(D):
            n[(s // P ** d) % P] += np.uint64(occ[s])
    return n


def threshold_after_update(o, dynamic):
    """The wavelet threshold under the theta the sweep's update has just drawn, from the checker alone.  The checker keeps the
    threshold its LAST ENUMERATION used - one update behind while the blocks are dynamic - and takes the one of its current
    theta where a sweep begins or the blocks are made static: token S does exactly that, and token D undoes its only other
    effect.  (No prior draw is pending right behind a sweep.)  Static blocks: the threshold stays what it was."""
    if dynamic:
        o.token("S")
        thr = o.threshold()
        o.token("D")
        return thr
    return o.threshold()


def row_of(o, prior, method, sweep, chain, D=1, P=None, dirichlet=DIRICHLET, dynamic=True):
    """(row[11], bound[11]) of the checker's state after a sweep; bound is 0 in the exact columns, NaN where the value is not finite"""
    K = o.K
    Pn = P if D > 1 else K
    trans, occ, sx, sxx, nterms = o.counts()
    theta = o.theta()
    mu, var = theta[0::2].astype(np.float64), theta[1::2].astype(np.float64)
    A, pi = o.transitions()
    A, pi = A.astype(np.float64), pi.astype(np.float64)
    n = terms_per_parameter(occ, K, D, Pn)
    assert np.array_equal(n, nterms[:Pn]), (n, nterms)
    nf = n.astype(np.float64)
    sx, sxx = sx[:Pn].astype(np.float64), sxx[:Pn].astype(np.float64)
    alpha, beta, mu0, nu = (float(v) for v in np.asarray(prior, np.float32))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        logA, logpi, logvar = np.log(A), np.log(pi), np.log(var)
        emit = np.concatenate([_times(0.5 * nf, np.log(2.0 * np.pi * var)), sxx / (2.0 * var), -2.0 * mu * sx / (2.0 * var),
                               np.where(n == 0, 0.0, nf * mu * mu / (2.0 * var))])
        if method == "M":
            path = _times(occ.astype(np.float64), logpi)
        else:
            path = np.concatenate([[logpi[int(o.states()[0])]], _times(trans.astype(np.float64), logA).reshape(-1)])
        ptheta = np.concatenate([-(alpha + 1.0) * logvar, -beta / var, -0.5 * logvar, -nu * (mu - mu0) ** 2 / (2.0 * var)])
        a = np.where(np.eye(K, dtype=bool), np.float64(np.float32(dirichlet["a_diag"])), np.float64(np.float32(dirichlet["a_off"])))
        ppath = np.concatenate([_times(a - 1.0, logA).reshape(-1), _times(np.full(K, np.float64(np.float32(dirichlet["pi_alpha"])) - 1.0), logpi)])
    row, bound = np.zeros(len(COLS)), np.zeros(len(COLS))
    row[0], row[1] = sweep, 1.0 if method == "M" else 0.0
    for col, addends, sign in ((2, emit, -1.0), (3, path, 1.0), (4, ptheta, 1.0), (5, ppath, 1.0)):
        total, bound[col] = _total(addends)
        row[col] = sign * total
    row[6] = 1.0 + float(int(trans.sum()) - int(np.trace(trans)))
    row[7] = float(o.num_blocks())
    row[8] = float(np.count_nonzero(occ))
    row[9] = float(np.float32(threshold_after_update(o, dynamic)))
    row[10] = float(chain)
    return row, bound


def walk(o, prior, scheme, chain=0, D=1, P=None, every=1, sweeps_before=0, visit=None):
    """the checker through the scheme one sweep per call: (rows[n, 11], bounds[n, 11]) of the sweeps whose number is a multiple of
    `every`.  visit(o, method, sweep, row): called after every sweep that leaves a row"""
    rows, bounds = [], []
    sweep = sweeps_before
    dynamic = True
    for tok in scheme:
        if isinstance(tok, str):
            o.token(tok)
            dynamic = False if tok == "S" else True if tok == "D" else dynamic
            continue
        m, n, _t = tok
        for _ in range(n):
            o.iterate(m, 1, 0)
            sweep += 1
            if sweep % every == 0:
                r, b = row_of(o, prior, m, sweep, chain, D, P, dynamic=dynamic)
                rows.append(r)
                bounds.append(b)
                if visit is not None:
                    visit(o, m, sweep, r)
    return np.array(rows).reshape(-1, len(COLS)), np.array(bounds).reshape(-1, len(COLS))


_EXPECTED = {}


def expected(name, case, chain=0, every=1):
    """(rows, bounds, blocks, states, theta of the checker's last sweep) of a named case: computed once per process, never changed"""
    key = (name, chain, every)
    if key not in _EXPECTED:
        o, prior = checker(case, chain=chain)
        try:
            rows, bounds = walk(o, prior, case["scheme"], chain=chain, D=case["D"], P=case["P"], every=every)
            _EXPECTED[key] = (rows, bounds, o.blocks().copy(), o.states().copy(), o.theta().copy())
        finally:
            o.close()
    rows, bounds, blocks, states, theta = _EXPECTED[key]
    return rows.copy(), bounds.copy(), blocks, states, theta


def kind(v):
    """0 finite, 1 +inf, 2 -inf, 3 NaN"""
    v = np.asarray(v, np.float64)
    return np.where(np.isnan(v), 3, np.where(np.isposinf(v), 1, np.where(np.isneginf(v), 2, 0)))


def assert_rows(got, want, bounds, what=""):
    """a chain's history() against the helper's rows: the exact columns bit for bit, columns 2-5 under their bound (the largest
    observed error is printed next to it), non-finite entries of the same kind"""
    got = np.asarray(got, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    for col in EXACT:
        assert np.array_equal(got[:, col].view(np.uint64), want[:, col].view(np.uint64)), (what, COLS[col], got[:, col][:6], want[:, col][:6])
    for col in BOUNDED:
        assert np.array_equal(kind(got[:, col]), kind(want[:, col])), (what, COLS[col], got[:, col], want[:, col])
        fin = np.isfinite(want[:, col])
        if not fin.any():
            print("%s: %s has no finite entry" % (what, COLS[col]))
            continue
        err = np.abs(got[fin, col] - want[fin, col])
        worst = int(np.argmax(err - bounds[fin, col]))
        print("%s: %s largest error %.3e; closest to its bound: error %.3e, bound %.3e; %d of %d rows finite"
              % (what, COLS[col], err.max(), err[worst], bounds[fin, col][worst], int(fin.sum()), len(fin)))
        assert np.all(err <= bounds[fin, col]), (what, COLS[col], worst, err[worst], bounds[fin, col][worst])


def same_bits(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def loglik_from_blocks(starts, sum_x, sum_xx, states, mu, var, A, pi, self_trans=True):
    """ll_emit + ll_path of an FB sweep block by block (D = 1): (value, sum |addend|) - the MEANING of columns 2 + 3, from the
    sweep's blocks, block statistics and states instead of the per-state sums the row is made of"""
    starts = np.asarray(starts, np.int64)
    q = np.asarray(states, np.int64)
    length = np.diff(starts).astype(np.float64)
    mu, var = np.asarray(mu, np.float64)[q], np.asarray(var, np.float64)[q]
    A, pi = np.asarray(A, np.float64), np.asarray(pi, np.float64)
    sx, sxx = np.asarray(sum_x, np.float64), np.asarray(sum_xx, np.float64)
    with np.errstate(divide="ignore"):
        logA, logpi = np.log(A), np.log(pi)
    emit = [-0.5 * length * np.log(2.0 * np.pi * var), -sxx / (2.0 * var), 2.0 * mu * sx / (2.0 * var), -length * mu * mu / (2.0 * var)]
    # (the count pass starts with `prev = 0` like the reference: it counts a transition from state 0 into the first block, and the
    # conjugate update of A uses it - so does the row, whose N is what hml_get_counts returns)
    path = [np.array([logpi[q[0]], logA[0, q[0]]]), logA[q[:-1], q[1:]]]
    if self_trans:
        path.append(_times(length - 1.0, logA[q, q]))
    a = np.concatenate(emit + path)
    return math.fsum(a), float(np.sum(np.abs(a)))


# ---- hml_history_stats, restated ----
def stats(x):
    """dict(rhat, ess, chain_mean, chain_sd, n_nonfinite) of x[n_chains, n] by the formulas of include/hml.h; ValueError when a half
    has fewer than 4 values"""
    x = np.atleast_2d(np.asarray(x, np.float64))
    C, n = x.shape
    h = n // 2
    if h < 4:
        raise ValueError("h < 4")
    fin = np.isfinite(x)
    out = dict(n_nonfinite=int((~fin).sum()), rhat=float("nan"), ess=float("nan"))
    out["chain_mean"] = np.array([x[c][fin[c]].mean() if fin[c].any() else np.nan for c in range(C)])
    out["chain_sd"] = np.array([x[c][fin[c]].std(ddof=1) if fin[c].sum() >= 2 else np.nan for c in range(C)])
    if out["n_nonfinite"]:
        return out
    seq = np.concatenate([np.stack([x[c, :h], x[c, n - h:]]) for c in range(C)])      # m = 2 C sequences of length h
    m = 2 * C
    mean_j = seq.mean(axis=1)
    W = float(seq.var(axis=1, ddof=1).mean())
    B = h / (m - 1.0) * float(((mean_j - mean_j.mean()) ** 2).sum())
    var_plus = (h - 1.0) / h * W + B / h
    if not W > 0:
        return out
    out["rhat"] = math.sqrt(var_plus / W)
    d = seq - mean_j[:, None]

    def rho(t):
        acov = (d[:, : h - t] * d[:, t:]).sum(axis=1) / h
        return 1.0 - (W - float(acov.mean())) / var_plus
    total, prev, k = 0.0, 0.0, 0
    while 2 * k + 1 <= h - 1:
        P = 1.0 + rho(1) if k == 0 else rho(2 * k) + rho(2 * k + 1)
        if P < 0:
            break
        if k > 0:
            P = min(P, prev)
        total += P
        prev = P
        k += 1
    out["ess"] = m * h / (-1.0 + 2.0 * total)
    return out


def ar1(phi, chains, n, seed, shift=None):
    """AR(1) series of unit innovation variance from a fixed seed, started in the stationary law: float64 [chains, n]"""
    rng = np.random.RandomState(seed)
    e = rng.standard_normal((chains, n))
    x = np.empty((chains, n))
    x[:, 0] = e[:, 0] / math.sqrt(1.0 - phi * phi)
    for i in range(1, n):
        x[:, i] = phi * x[:, i - 1] + e[:, i]
    if shift is not None:
        x[shift[0]] += shift[1] * x.std()
    return x

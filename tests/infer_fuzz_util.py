"""TEST INFRASTRUCTURE: the exact-inference passes of hml_infer.hip against their restatements for one host thread - the plumbing
the hostile tests share (tests/test_gpu_infer_hostile.py) and a randomised differential run over data kinds, sizes, numbers of
states, block regimes, parameters and geometries (tests/test_gpu_infer_fuzz.py runs a fixed-seed sample, tools/fuzz_infer.py as
many as asked).  Every pass goes through the check functions of its own test module, fed the GPU's own block_stats(), blocks(),
theta() and transitions(); the one NaN translation is tests/words_util.expected_words.  generate() is a pure
function of (n, seed): tests/test_infer_fuzz_cpu.py shows without a GPU what the sample covers."""
import contextlib
import os
import time

import numpy as np

from tests import em_util as eu
from tests import hostile_inputs as hi
from tests import infer_cases as ic
from tests import oracle_lib as ol
from tests import pairs_util as pz
from tests import posterior_util as pu
from tests import sample_util as su
from tests import viterbi_util as vu
from tests.words_util import expected_words, same_or_translated

f32 = np.float32
PASSES = ("viterbi", "posterior", "counts", "fits", "em_many", "pairs", "sample")
N_PATHS = 8
NIG4 = np.array([2.0, 1.0, 0.0, 1.0], f32)      # the prior where the automatic one is refused, and under planted parameters


def build_programs(directory):
    """the plain builds of the five stand-alone programs: pass -> path; "sample" -> (path, a directory for its paths file)"""
    out = {}
    for name, util in (("viterbi", vu), ("posterior", pu), ("em", eu), ("pairs", pz), ("sample", su)):
        sub = os.path.join(str(directory), name)
        os.makedirs(sub, exist_ok=True)
        out[name] = util.build_programs(sub, sanitized=False)["plain"]
    out["sample"] = (out["sample"], os.path.join(str(directory), "sample"))
    return out


@contextlib.contextmanager
def device_nans(g):
    """Inside, the words the programs print for chain g reach the check functions of the passes' test modules as
    words_util.expected_words has them: where a program holds the host's made NaN and the chain the device's, the device's.
    The words that can be no number at all: e, m, c and the log-likelihood (alpha, beta, gamma, xi, p and r fall back to
    numbers behind a degenerate block); a fit's trace and parameters are compared in check_fits."""
    run_case, run_program = pu.run_case, eu.run_program

    def posterior(exe, case, want_rows=True):
        out = run_case(exe, case, want_rows)
        e, m, _, c, _ = g.posterior_terms()
        for key, dev, bits in (("e", pu.words32(e), 32), ("m", pu.words32(m), 32), ("c", pu.words(c), 64), ("loglik", pu.words([g.posterior()[1]]), 64)):
            if key in out:
                out[key] = expected_words(out[key], dev, bits)
        return out

    def em(exe, mode, case, **kw):
        out = run_program(exe, mode, case, **kw)
        if mode == "estep":
            out["loglik"] = expected_words(out["loglik"], pu.words([g.expected_counts()["loglik"]]))
        return out

    pu.run_case, eu.run_program = posterior, em
    try:
        yield
    finally:
        pu.run_case, eu.run_program = run_case, run_program


# ---------------------------------------------------------------------------------------------- the passes
def check_fits(programs, g, self_trans, what):
    """em_fit of 3 steps from the chain's parameters, without and with the prior: trace, steps, reason, kept and the parameters
    left in the chain; the chain gets its parameters back"""
    from tests import test_gpu_em as te
    case = pu.chain_case(g, self_trans)
    mv, (A, pi) = g.theta(), g.transitions()
    reasons = []
    for prior_on in (False, True):
        g.set_parameters(mv, A, pi)
        want = eu.run_program(programs["em"], "fit", case, use_prior=prior_on, prior=te.prior(g), max_steps=3)
        trace, steps, reason, kept = g.em_fit(3, use_prior=prior_on)
        w = (what, prior_on)
        assert same_or_translated(pu.words(trace), want["trace"]), (w, trace, want["trace"].view(np.float64))
        assert (steps, reason, kept) == (want["steps"], want["reason"], want["kept"]), w
        A2, pi2 = g.transitions()
        assert same_or_translated(pu.words32(g.theta()), want["mean_var"], 32), w
        assert same_or_translated(pu.words32(A2), want["A"], 32) and same_or_translated(pu.words32(pi2), want["pi"], 32), w
        reasons.append(reason)
    g.set_parameters(mv, A, pi)
    return reasons


def check_sample(programs, g, self_trans, what):
    """N_PATHS paths with every count, and the region histograms at the edge regions: the words (the bounds of
    tests/sample_util.invariants hold for ordinary numbers only - not for a wrapped score, not behind a degenerate block)"""
    from tests import test_gpu_sample as ts
    regions = pz.edge_regions(g.blocks(), np.random.default_rng(5), n_random=3)
    want = ts.reference(programs["sample"], g, N_PATHS, 7, 0, self_trans, regions)
    got = ts.check_sample(g, want, N_PATHS, 7, 0, what)
    reg = g.posterior_sample_regions(regions[0], regions[1], N_PATHS, seed=7, first=0, max_breaks=ts.H)
    su.same(reg, want, su.REGION_KEYS, what)
    su.same(reg, su.region_counts(got["paths"], g.K, g.blocks(), regions[0], regions[1], ts.H), su.REGION_KEYS, what)
    return want


def check_pass(hml, programs, g, pass_, self_trans=True, what=None):
    """one pass of PASSES against its program (inside device_nans(g)); returns what tests/infer_cases.flags reads of it"""
    from tests import test_gpu_em as te
    from tests import test_gpu_em_many as tm
    from tests import test_gpu_pairs as tp
    from tests import test_gpu_posterior as tpo
    from tests import test_gpu_viterbi as tv
    if pass_ == "viterbi":
        want = tv.check(programs["viterbi"], g, self_trans, what)
        plain = vu.path_score(want["path"].tolist(), want["emit"].tolist(), want["trans"].tolist(), want["init"].tolist())
        return dict(emit=want["emit"], score=want["score"], score_plain=plain)
    if pass_ == "posterior":
        want = tpo.check(programs["posterior"], g, self_trans, what)
        return dict(degenerate=want["degenerate"], loglik=float(want["loglik"].view(np.float64)[0]), e=want["e"].view(np.float32))
    if pass_ == "counts":
        want = te.check(programs["em"], g, self_trans, what)
        K, D = g.K, g.D
        return dict(xi_degenerate=want["xi_degenerate"], occ=want["occ"].view(np.float64), sx=want["sx"].view(np.float64).reshape(K, D),
                    sxx=want["sxx"].view(np.float64).reshape(K, D))
    if pass_ == "fits":
        return dict(reasons=check_fits(programs, g, self_trans, what))
    if pass_ == "em_many":
        tm.check_batch(g, g.em_starts(3, 7), max_steps=3, self_trans=self_trans, what=what)
        return {}
    if pass_ == "pairs":
        want = tp.check(hml, programs["pairs"], g, self_trans, what, n_random=20)
        return dict(pair_degenerate=want["pair_degenerate"])
    assert pass_ == "sample"
    return dict(sample_degenerate=check_sample(programs, g, self_trans, what)["sample_degenerate"])


# ---------------------------------------------------------------------------------------------- configurations
KS = (2, 3, 5, 8, 9, 16, 17, 20, 64)
TS = tuple(t for t in hi.FUZZ_T if t <= 4097)
KINDS = ("trace", "scale2", "scale10", "offset", "depth", "plateaus", "plateaus_noise", "alternation", "arange", "rounded", "spikes")
PARAMS = ("chain", "unit", "denormal")
SAMPLE = (56, 20261301)      # (configurations, seed) of the suite's sample


def _draw_data(rng, T):
    """(kind, float32[T]): ol.trace one time in four, else a member of hostile_inputs.fuzz_draw"""
    if rng.random() < 0.25:
        return "trace", ol.trace(max(T, 16), 3, int(rng.integers(1, 1000)))[:T].copy()
    desc, x = hi.fuzz_draw(rng, T=T)
    return desc.split("^")[0].split("*")[0].split("+")[0].split("=")[0], x


def generate(n, seed, only=None):
    """the configurations 0 ... n - 1 of the seed (or the one `only` names), each from a generator of its own"""
    out = []
    for i in ([only] if only is not None else range(n)):
        rng = np.random.default_rng([seed, i])
        two = rng.random() < 0.15
        c = dict(i=i, seed=seed, T=int(rng.choice(TS)), dims=(2, 2) if two else None, K=4 if two else int(rng.choice(KS)), data_seed=int(rng.integers(1 << 31)),
                 self_trans=bool(rng.random() < 0.7), every_position=bool(rng.random() < 0.6), sweeps=int(rng.integers(0, 6)),
                 zeros=bool(rng.random() < 0.4), zero_seed=int(rng.integers(1 << 31)), params=PARAMS[int(rng.choice(3, p=[0.3, 0.2, 0.5]))],
                 chain_seed=int(rng.integers(1, 1000)),
                 geometry={p: (int(rng.choice([1, 4, 64, 1024])), int(rng.choice([4, 64, 512])), int(rng.choice([0, 1, 8]))) for p in ("viterbi", "posterior", "sample")})
        if c["T"] == 1:
            c["sweeps"] = 0           # (a trace of one position is the context with one block: it has no sweep)
        c["kind"] = data(c)[0]
        out.append(c)
    return out


def data(c):
    """(kind, the float32 input: T positions, the dimensions interleaved)"""
    rng = np.random.default_rng(c["data_seed"])
    if not c["dims"]:
        return _draw_data(rng, c["T"])
    parts = [_draw_data(rng, c["T"]) for _ in range(c["dims"][0])]
    return parts[0][0], np.stack([x for _, x in parts], axis=1).reshape(-1).astype(f32)


def planted(c, theta):
    """the emission parameters of the configuration: the chain's own, unit-scale ones, or those with every variance but the first
    at the smallest float denormal - such a state's E is inf - inf = NaN where the position lies between 0 and twice its mean,
    and -inf elsewhere: blocks that are reset next to blocks that are not"""
    if c["params"] == "chain":
        return theta
    P = c["dims"][1] if c["dims"] else c["K"]
    mv = ic.mean_var(ic.levels(P), 0.04)
    if c["params"] == "denormal":
        mv[3::2] = ic.DENORMAL
    return mv


def with_zeros(c, A, pi):
    """zeros off the diagonal of A and in pi (the diagonal stays positive: 0 x -inf is no number, tests/test_gpu_posterior.py),
    rows scaled back to sum 1 in float"""
    if not c["zeros"]:
        return A, pi
    K = c["K"]
    rng = np.random.default_rng(c["zero_seed"])
    keep = rng.random((K, K)) < 0.6
    np.fill_diagonal(keep, True)
    A = np.where(keep, np.asarray(A, f32).reshape(K, K), f32(0))
    keep_pi = rng.random(K) < 0.6
    keep_pi[int(rng.integers(K))] = True
    pi = np.where(keep_pi, np.asarray(pi, f32), f32(0))
    with np.errstate(all="ignore"):
        rows, total = A.sum(1, keepdims=True, dtype=f32), pi.sum(dtype=f32)
        A = np.where(rows > 0, A / rows, A).astype(f32)
        pi = (pi / total).astype(f32) if total > 0 else pi
    return A, pi


def ideal_case(c):
    """where the configuration's case does not depend on a chain's sweeps - every position a block, planted parameters - the case
    with the statistics summed on the host, transitions sticky before the zeros; else None"""
    if c["params"] == "chain" or not c["every_position"]:
        return None
    K, (D, P) = c["K"], c["dims"] or (1, c["K"])
    A, pi = with_zeros(c, ic.sticky(K), ic.uniform(K))
    with np.errstate(all="ignore"):
        return ic.ideal_case(dict(x=data(c)[1], K=K, D=D, P=P, self_trans=c["self_trans"], block=1, mean_var=planted(c, None), A=A, pi=pi))


def line_of(c):
    return "%3d: %-14s T %5d K %2d%s %s %s sweeps %d params %-8s%s geometry %s" % (
        c["i"], c["kind"], c["T"], c["K"], " D 2" if c["dims"] else "", "self" if c["self_trans"] else "free", "every" if c["every_position"] else "blocks",
        c["sweeps"], c["params"], " zeros" if c["zeros"] else "", " ".join("%d/%d/%d" % c["geometry"][p] for p in ("viterbi", "posterior", "sample")))


# ---------------------------------------------------------------------------------------------- the run
def build_chain(hml, c):
    _, x = data(c)
    g = hml.Chain(device=0, seed=c["chain_seed"])
    if c["dims"]:
        g.set_dimensions(*c["dims"])
    g.load(x)
    if c["every_position"]:
        g.scale_weights(1e9)
    sweeps = c["sweeps"]
    try:
        g.em_nig4 = g.autoprior(0.2, 0.9)
    except hml.HmlError:              # constant data, one position: no automatic prior, and no sweep either
        g.em_nig4, sweeps = NIG4, 0
    g.set_model(c["K"], g.em_nig4, self_trans=c["self_trans"])
    g.sample_prior()
    if sweeps:
        g.iterate("F", sweeps, 0)
        g.sync()
    else:
        g.create_blocks(0.0 if c["every_position"] else g.threshold())
    A, pi = g.transitions()
    if c["params"] != "chain" or c["zeros"]:
        g.set_parameters(planted(c, g.theta()), *with_zeros(c, A, pi))
    for p, (W, L, rounds) in c["geometry"].items():
        g.set_option(p + "_W", W)
        g.set_option(p + "_L", L)
        g.set_option(p + "_rounds", rounds)
    return g


def run_configuration(hml, programs, c):
    g = build_chain(hml, c)
    try:
        with device_nans(g):
            seen = {}
            for pass_ in PASSES:
                seen.update(check_pass(hml, programs, g, pass_, c["self_trans"], (line_of(c), pass_)))
        return seen
    finally:
        g.close()


def fuzz_infer(hml, programs, n, seed, log=None, only=None):
    """runs the configurations; returns how many ran (every one of them identical, or an assertion names the first that is not:
    python tools/fuzz_infer.py --seed S --only I)"""
    done = 0
    for c in generate(n, seed, only):
        t0 = time.perf_counter()
        seen = run_configuration(hml, programs, c)
        done += 1
        if log:
            log("%s: degenerate %d  %.1f s" % (line_of(c), seen["degenerate"], time.perf_counter() - t0))
    return done

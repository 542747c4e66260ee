"""TEST INFRASTRUCTURE: the chains of the breakpoint tests, shared by tests/test_breaks_cpu.py (which shows on the CPU checker
that every consensus case is non-vacuous) and tests/test_gpu_breaks.py (which runs them on the GPU).

CASES: name -> dict(T, K, seed, scheme, trace, D, P, compat, env).  `env`: environment of the GPU chain only (launch
geometry; the checker has none).  CONSENSUS: the (window, P) pairs of every case; min_count = max(1, ceil(P N)), the
driver's rule (breaks_util.min_count_of).  arbitrary_cuts(T): cuts for hml_levels_on_segments that ignore the levels'
boundaries."""
import numpy as np

from tests import oracle_lib as ol

MIXED = [("M", 6, 2), "S", "P", ("F", 6, 0), ("F", 9, 3), "D", ("F", 4, 1)]   # the mixed scheme of tests/test_gpu_levels.py


def _gauss(T, levels, seed):
    return lambda: ol.trace(T, levels, seed)


def _mv(T, P, D, seed):
    return lambda: np.stack([ol.trace(T, P, seed + d) for d in range(D)], axis=1).reshape(-1)


def _case(T, K, seed, scheme, trace, D=1, P=None, compat=False, env=()):
    return dict(T=T, K=K, seed=seed, scheme=scheme, trace=trace, D=D, P=P, compat=compat, env=dict(env))


CASES = {
    "k2": _case(60000, 2, 42, [("F", 30, 1)], _gauss(60000, 2, 7)),
    "k5": _case(100000, 5, 42, [("F", 40, 2)], _gauss(100000, 5, 7)),
    "k10": _case(50000, 10, 42, [("F", 24, 2)], _gauss(50000, 10, 7)),
    "k20_wide": _case(60000, 20, 42, [("F", 24, 2)], _gauss(60000, 6, 7)),          # more than 16 states: sweep_wide
    "compat_k4": _case(20000, 4, 3, [("M", 12, 1), ("F", 20, 2)], _gauss(20000, 4, 7), compat=True),
    "mv_c22": _case(40000, 4, 6, [("M", 5, 1), ("F", 30, 2)], _mv(40000, 2, 2, 9), D=2, P=2),
    "k4_mixed": _case(20000, 4, 42, MIXED, _gauss(20000, 4, 7)),
    # 1.4 positions per block, and the forward geometry of weakly compressed sweeps forced on from the first block
    "depth_weak": _case(60000, 5, 17, [("M", 4, 0), ("F", 20, 2)], lambda: ol.synth_depth(60000, seed=5),
                        env={"HML_DENSE_MIN_BLOCKS": "1"}),
}

CONSENSUS = [(2, 0.5), (16, 0.75), (64, 1.0)]
DENSE_WINDOWS = [0, 1, 16]


def checker(case, chain=0, seed=None):
    c = CASES[case] if isinstance(case, str) else case
    mode = (ol.RNG_MT, ol.MATH_LIBM, ol.REDUCE_REF) if c["compat"] else (ol.RNG_CTR, ol.MATH_DEV, ol.REDUCE_DEV)
    o = ol.OracleChain(K=c["K"], seed=c["seed"] if seed is None else seed, chain=chain, rng=mode[0], math=mode[1], reduce=mode[2],
                       weight_mult=c.get("weight_mult", 1.0))
    if c["D"] > 1:
        o.set_dimensions(c["D"], c["P"])
    o.load(c["trace"]() if callable(c["trace"]) else c["trace"])
    o.autoprior()
    o.init_model()
    return o


def checker_sweeps(o, scheme, recording=None, marginals=False):
    """the checker through the scheme one sweep per call: (starts, states, means) of every recorded sweep.
    `recording`: per scheme token, whether the recording under test is on (None: always).  `marginals`: the checker counts
    every recorded sweep into its own state marginals as well (a call of one sweep with thinning 1: the same chain)"""
    sweeps = []
    for k, tok in enumerate(scheme):
        if isinstance(tok, str):
            o.token(tok)
            continue
        m, n, t = tok
        for i in range(n):
            recorded = t > 0 and (i + 1) % t == 0
            o.iterate(m, 1, 1 if (marginals and recorded) else 0)
            if recorded and (recording is None or recording[k]):
                sweeps.append((o.blocks().copy(), o.states().copy(), o.theta()[0::2].copy()))
    return sweeps


def arbitrary_cuts(T):
    """ascending cuts in (0, T) on a grid that knows nothing of the chain: every T / 37-th position, shifted"""
    step = max(1, T // 37)
    cuts = np.arange(step // 2 + 1, T, step, dtype=np.int64)
    return cuts[(cuts > 0) & (cuts < T)]

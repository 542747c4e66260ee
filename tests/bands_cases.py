"""TEST INFRASTRUCTURE: the chains of the level-band tests, shared by tests/test_bands_cpu.py (which shows on the CPU checker
that every case is non-vacuous) and tests/test_gpu_bands.py (which runs them on the GPU).

CASES: name -> dict(T, K, seed, scheme, trace, D, P, compat, edges).  The edges lie between the levels of the trace
(ol.LEVELS): whole numbers for 3, 5 and the C 2 2 traces, halves for 4, 6, 10 and 16 levels.  RANK_CASES: the cases whose calls
are compared at rank 1, ceil(N / 2) and N as well."""
import json
import os

import numpy as np

from tests import breaks_cases as bc
from tests import oracle_lib as ol

MIXED = bc.MIXED
WIDE40 = [("M", 4, 1), "S", "P", ("F", 8, 2), "D", ("F", 3, 1)]
CN = (-0.5, 0.5)                                     # loss / neutral / gain
FINE9 = tuple(-2.25 + 0.5 * j for j in range(9))


def _case(T, K, seed, scheme, trace, edges, D=1, P=None, compat=False):
    return dict(T=T, K=K, seed=seed, scheme=scheme, trace=trace, D=D, P=P, compat=compat, edges=tuple(edges), env={})


def _gauss(T, K, seed=7):
    return lambda: ol.trace(T, K if K in ol.LEVELS else 6, seed)


def _golden(case):
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "manifest.json")) as f:
        return json.load(f)[case]


def _compat_k4():
    m = _golden("k4_mixed_scheme")
    assert m["flags"] == "-s 4 -R 3 -i M 50 5 D F 60 2 P M 10 1 S F 30 1"
    return _case(m["T"], 4, 3, [("M", 50, 5), "D", ("F", 60, 2), "P", ("M", 10, 1), "S", ("F", 30, 1)],
                 lambda: ol.trace(m["T"], m["trace_levels"], m["data_seed"]), (0.0,), compat=True)


def _compat_mv():
    m = _golden("mv_c22")
    assert m["flags"] == "-s C 2 2 -R 5 -i F 50 1" and m["dims"] == 2
    return _case(m["T"], 4, 5, [("F", 50, 1)],
                 lambda: np.stack([ol.trace(m["T"], m["trace_levels"], m["data_seed"] + d) for d in range(2)], axis=1).reshape(-1),
                 (0.5,), D=2, P=2, compat=True)      # (the first recorded sweep has both parameters below 0.5)


CASES = {
    "k3": _case(100000, 3, 42, [("F", 30, 1)], _gauss(100000, 3), CN),
    "k5": _case(200000, 5, 42, [("F", 25, 5)], _gauss(200000, 5), CN),
    "k5_fine": _case(200000, 5, 42, [("F", 25, 5)], _gauss(200000, 5), FINE9),
    "k10": _case(50000, 10, 42, [("F", 10, 2)], _gauss(50000, 10), (-2.0, 0.0, 2.0)),
    "k16": _case(30000, 16, 42, [("F", 6, 2)], _gauss(30000, 16), (-4.0, -1.0, 1.0, 4.0)),
    "k20_wide": _case(60000, 20, 42, [("F", 12, 3)], _gauss(60000, 20), (-1.0, 1.0)),      # more than 16 states: sweep_wide
    "k40_wide": _case(30000, 40, 42, WIDE40, _gauss(30000, 40), (-1.0, 1.0)),
    "k4_mixed": _case(20000, 4, 42, MIXED, _gauss(20000, 4), (-1.0, 1.0)),
    "k20_mixed": _case(30000, 20, 42, MIXED, _gauss(30000, 20), (-1.0, 1.0)),
    # read depth around 15 per copy: the copy-number cut-offs
    "depth": _case(300000, 5, 17, [("M", 10, 0), ("F", 30, 3)], lambda: ol.synth_depth(300000, seed=5), (7.5, 15.0, 22.5, 30.0)),
    # `-s C 2 2`: two parameters near -1 and 1 shared by four states over two dimensions, ONE edge.  An edge between the two
    # levels would keep the parameters in different bands in every sweep; this one lies inside the spread of the upper
    # parameter's recorded means (1.0007 ... 1.0025 on the checker), so in some sweeps all four states share band 0
    "mv_c22": _case(40000, 4, 6, [("M", 5, 1), ("F", 15, 2)], bc._mv(40000, 2, 2, 9), (1.0015,), D=2, P=2),
    "compat_k4": _compat_k4(),
    "compat_mv": _compat_mv(),
}

RANK_CASES = ["k3", "mv_c22"]      # D = 1 and D = 2


def checker(case, chain=0, seed=None):
    return bc.checker(CASES[case] if isinstance(case, str) else case, chain=chain, seed=seed)


checker_sweeps = bc.checker_sweeps

_SWEEPS = {}


def sweeps_of(case):
    """the checker's recorded sweeps of a named case, computed once per process and never changed"""
    if case not in _SWEEPS:
        o = checker(case)
        try:
            _SWEEPS[case] = tuple(checker_sweeps(o, CASES[case]["scheme"]))
        finally:
            o.close()
    return list(_SWEEPS[case])

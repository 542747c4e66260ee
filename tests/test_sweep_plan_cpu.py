"""Which kernels a sweep of the default path launches is decided by one pure function, hml_plan_sweep
(hammlet_amd/csrc/hml_sweep_plan.h: no HIP, a host compiler builds it).  Which path a sweep takes never changes its results, so
the bit-for-bit GPU tests cannot see a sweep that takes the wrong one: this test holds the decision itself.  A stand-alone
program (tests/fixtures/sweep_plan_main.cpp) prints the plan for rows of inputs; the expected rows below are written out from
the rules - thresholds 2^18 (mid) and 2^22 (many blocks), the float stream from hint * 24 > T, rows<true> from
(hint - 1024) * 8 >= 9 T - not from the function's output."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T8 = 10 ** 8

# the plan of the default sweep, strongly compressed: chunks of 4, no plane of rescale factors, fused block kernel wanted
SPARSE = dict(geo="sparse", L=4, lshift=2, cstride=0, mix=0, spread=0, gsc=0, trellis=0, fused=1, scan="summary", first="rows<false>", counts="plain", levels=1, fs=0, mb=0)
MID = dict(SPARSE, geo="mid", L=8, lshift=3)
MID_FS = dict(MID, fused=0, scan="flags", fs=1)                       # the float stream: no fused kernel, flags staged
DENSE = dict(geo="dense", L=16, lshift=4, cstride=0, mix=0, spread=0, gsc=1, trellis=1, fused=0, scan="flags", first="rows<false>", counts="dense", levels=2, fs=1, mb=1)


def row(hint, T=T8, D=1, mix=0, alone=1, expired=0, **knobs):
    return " ".join([str(hint), str(T), str(D), str(mix), str(alone), str(expired)] + ["%s=%d" % kv for kv in knobs.items()])


CASES = [
    # (name, input row, expected plan)
    ("hint 0", row(0), SPARSE),
    ("hint 2^18 - 1", row(262143), SPARSE),
    ("hint 2^18", row(262144), MID),
    ("hint 4166666: x 24 = 99 999 984 <= T", row(4166666), MID),
    ("hint 4166667: x 24 = 100 000 008 > T", row(4166667), MID_FS),
    ("hint 4166667, stage_bits off", row(4166667, stage_bits=0), dict(MID_FS, scan="float")),
    ("hint 4166667, summary_always", row(4166667, summary_always=1), MID),
    ("hint 2^22 - 1", row(4194303), MID_FS),
    ("hint 2^22", row(4194304), DENSE),
    ("hint 2^22, tre_fused off", row(4194304, tre_fused=0), dict(DENSE, trellis=0)),
    ("hint 2^22, tre_rows off", row(4194304, tre_rows=0), dict(DENSE, first="tile")),
    ("hint 112501023: (hint - 1024) x 8 = 899 999 992 < 9 T", row(112501023), DENSE),
    ("hint 112501024: (hint - 1024) x 8 = 9 T", row(112501024), dict(DENSE, first="rows<true>")),
    ("mixture at 2^22", row(4194304, mix=1), dict(DENSE, trellis=0, mix=1)),
    ("mixture at hint 0", row(0, mix=1), dict(SPARSE, mix=1)),
    ("params_spread on", row(0, params_spread=1), dict(SPARSE, spread=1)),
    ("layout stride 1024 (set with the model)", row(262144, cstride=1024), dict(MID, cstride=1024)),
    ("D = 2, hint 0", row(0, D=2), dict(SPARSE, fused=0, counts="multivariate")),
    ("D = 2, hint 2^18", row(262144, D=2), dict(MID, fused=0, counts="multivariate")),
    ("D = 2, hint 2^22", row(4194304, D=2), dict(DENSE, trellis=0, counts="multivariate")),
    ("not alone on the device", row(0, alone=0), dict(SPARSE, fused=0)),
    ("wait expired", row(0, expired=1), dict(SPARSE, fused=0)),
    ("wait expired, fused_keep", row(0, expired=1, fused_keep=1), SPARSE),
    ("fused_blocks off", row(0, fused_blocks=0), dict(SPARSE, fused=0)),
    ("use_keys off at hint 1000", row(1000, use_keys=0), dict(SPARSE, fused=0, scan="float")),
    ("L[sparse] = 8, hint 2^18", row(262144, L_sparse=8), dict(SPARSE, L=8, lshift=3)),
    ("L[sparse] = 8, hint 2^22 - 1", row(4194303, L_sparse=8), dict(SPARSE, L=8, lshift=3, fused=0, scan="flags", fs=1)),
    ("mid_min_blocks = 200 at hint 200", row(200, mid_min_blocks=200), MID),
    ("mid_min_blocks = 200 at hint 199", row(199, mid_min_blocks=200), SPARSE),
    ("late_rescale off", row(0, late_rescale=0), dict(SPARSE, gsc=1)),
    ("short trace, hint 5000: x 24 > 100 000", row(5000, T=100000), dict(SPARSE, fused=0, scan="flags", fs=1)),
    ("dense_min_blocks = 1 at hint 0", row(0, dense_min_blocks=1), SPARSE),
    ("dense_min_blocks = 1 at hint 2000, T = 10^5", row(2000, T=100000, dense_min_blocks=1), dict(DENSE, fused=1, scan="summary", fs=0)),
]


def build(tmp_path, *flags):
    exe = str(tmp_path / ("sweep_plan" + "".join(flags).replace("=", "_").replace(",", "_")))
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *flags, "-I", os.path.join(REPO, "hammlet_amd", "csrc"), "-o", exe,
                    os.path.join(REPO, "tests", "fixtures", "sweep_plan_main.cpp")], check=True)
    return exe


def expected_line(p):
    # (the last column: the fields that operator== of two plans ignores - none, or a captured sweep could be replayed under another plan)
    return "%s %d %d %d %d %d %d %s %s %s %d %d %d | %d %d | %d %d | -" % (p["geo"], p["L"], p["lshift"], p["cstride"], p["gsc"], p["trellis"], p["fused"], p["scan"],
                                                                            p["first"], p["counts"], p["levels"], p["mix"], p["spread"], p["fs"], p["mb"], p["fs"], p["mb"])


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all")], ids=["plain", "sanitized"])
def test_sweep_plan_follows_the_rules(tmp_path, flags):
    """Every row's plan as the rules give it, the two predicates agree with the plan's own fields (the two columns before them) on
    every row, and two plans that differ in any one field compare unequal (last column).  Built a second time with the address and undefined-behaviour sanitizers and run stand-alone."""
    exe = build(tmp_path, *flags)
    r = subprocess.run([exe], input="".join(c[1] + "\n" for c in CASES), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = r.stdout.splitlines()
    assert len(got) == len(CASES)
    for (name, _, want), line in zip(CASES, got):
        assert line == expected_line(want), name

"""What a sweep of the reference-compatible mode and of the path for more than 16 states launches is decided by one pure
function, hml_plan_rtk (hammlet_amd/csrc/hml_rtk_plan.h: no HIP, a host compiler builds it).  Every chunk of these sweeps is
verified bit for bit, so the GPU parity tests cannot see a sweep that takes the wrong form: this test holds the decision itself.
A stand-alone program (tests/fixtures/rtk_plan_main.cpp) prints the plan for rows of inputs; the expected rows are written out
from the rules, not from the function's output:
  * state a lane: C = 1 when probed or a mixture sweep; compat_chunks > 1 chunks (at most 16384); compat_chunks = 0 and a hint
    from 8192 (reference-compatible) / 2048 (more than 16 states) on: hint / 64 chunks (at most 16384);
  * the count pass by state: reference-compatible, one dimension, T < 2^31, and compat_chunks > 1 or (0 and hint >= 8192) -
    whether the rows are probed or not;
  * a chunk a lane: more than 16 states unless wide_lanes = 0, probed, a mixture sweep or compat_chunks != 0; K rounded up to
    a multiple of 4; at most 131072 chunks up to 36 (padded) states and 65536 beyond, or wide_max_chunks (at most 131072);
    chunks of at least 4 blocks or the forced length; room = hint + hint / 4 + 1024;
  * the warm-up: compat_warmup > 0 that many blocks, < 0 none, 0 the model's adaptive one."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T6 = 10 ** 6

# the reference-compatible sweep below its threshold: one chunk, counts in block order
SEQ = dict(form="sequential", C=1, W="adaptive", by_state=0, exp="glibc", KC=3, pad=0, mix=0, max_chunks=0, min_L=0, room=0)
# more than 16 states, a state a lane (K = 20: loops over 32), and a chunk a lane at a hint of 5000
WSEQ = dict(SEQ, exp="dev", KC=32, pad=1)
LANES = dict(SEQ, form="lanes", exp="dev", KC=20, max_chunks=131072, min_L=4, room=5000 + 1250 + 1024)


def row(mode, hint, K=None, D=1, T=T6, mix=0, probes=0, **knobs):
    K = K if K is not None else (3 if mode == "compat" else 20)
    return " ".join([mode, str(K), str(D), str(T), str(mix), str(probes), str(hint)] + ["%s=%d" % kv for kv in knobs.items()])


CASES = [
    # (name, input row, expected plan)
    ("compat, hint 8191", row("compat", 8191), SEQ),
    ("compat, hint 8192: 128 chunks, by state", row("compat", 8192), dict(SEQ, form="chunked", C=128, by_state=1)),
    ("compat, hint 2 10^6: 31250 chunks clamped", row("compat", 2000000), dict(SEQ, form="chunked", C=16384, by_state=1)),
    ("compat, probed at 8192: one chunk, still by state", row("compat", 8192, probes=1), dict(SEQ, by_state=1)),
    ("compat, mixture at 8192: no filter, by state", row("compat", 8192, mix=1), dict(SEQ, mix=1, by_state=1)),
    ("compat_chunks 1 at 8192: sequential, block order", row("compat", 8192, compat_chunks=1), SEQ),
    ("compat_chunks 7 at hint 100", row("compat", 100, compat_chunks=7), dict(SEQ, form="chunked", C=7, by_state=1)),
    ("compat_chunks 7, probed", row("compat", 100, probes=1, compat_chunks=7), dict(SEQ, by_state=1)),
    ("compat_chunks 20000: clamped", row("compat", 100, compat_chunks=20000), dict(SEQ, form="chunked", C=16384, by_state=1)),
    ("compat_warmup -1: none", row("compat", 8192, compat_warmup=-1), dict(SEQ, form="chunked", C=128, by_state=1, W="0")),
    ("compat_warmup 0: adaptive", row("compat", 8192, compat_warmup=0), dict(SEQ, form="chunked", C=128, by_state=1)),
    ("compat_warmup 4", row("compat", 8192, compat_warmup=4), dict(SEQ, form="chunked", C=128, by_state=1, W="4")),
    ("compat, D = 2 at 8192: block order", row("compat", 8192, K=4, D=2), dict(SEQ, form="chunked", C=128, KC=4)),
    ("compat, D = 2, compat_chunks 7", row("compat", 100, K=4, D=2, compat_chunks=7), dict(SEQ, form="chunked", C=7, KC=4)),
    ("compat, T = 2^31 - 1", row("compat", 8192, T=2 ** 31 - 1), dict(SEQ, form="chunked", C=128, by_state=1)),
    ("compat, T = 2^31: block order", row("compat", 8192, T=2 ** 31), dict(SEQ, form="chunked", C=128)),
    ("compat, T = 2^31, compat_chunks 7", row("compat", 100, T=2 ** 31, compat_chunks=7), dict(SEQ, form="chunked", C=7)),
    ("compat ignores the wide knobs", row("compat", 8191, wide_lanes=0, wide_max_chunks=100, wide_lshift=5, wide_w0=8), SEQ),
    # the bucket of the state-a-lane dispatch, reference-compatible mode
    ("compat K 2", row("compat", 0, K=2), dict(SEQ, KC=2)),
    ("compat K 16", row("compat", 0, K=16), dict(SEQ, KC=16)),
    ("compat K 17", row("compat", 0, K=17), dict(SEQ, KC=32, pad=1)),
    ("compat K 32", row("compat", 0, K=32), dict(SEQ, KC=32, pad=1)),
    ("compat K 33", row("compat", 0, K=33), dict(SEQ, KC=64, pad=1)),
    ("compat K 36", row("compat", 0, K=36), dict(SEQ, KC=64, pad=1)),
    ("compat K 37", row("compat", 0, K=37), dict(SEQ, KC=64, pad=1)),
    ("compat K 64", row("compat", 0, K=64), dict(SEQ, KC=64, pad=1)),
    # more than 16 states, a state a lane
    ("wide, state a lane, hint 2047", row("wide", 2047, wide_lanes=0), WSEQ),
    ("wide, state a lane, hint 2048: 32 chunks", row("wide", 2048, wide_lanes=0), dict(WSEQ, form="chunked", C=32)),
    ("wide, state a lane, hint 8192: never by state", row("wide", 8192, wide_lanes=0), dict(WSEQ, form="chunked", C=128)),
    ("wide, state a lane, hint 2 10^6", row("wide", 2000000, wide_lanes=0), dict(WSEQ, form="chunked", C=16384)),
    ("wide, state a lane, K 2", row("wide", 0, K=2, wide_lanes=0), dict(WSEQ, KC=32)),
    ("wide, state a lane, K 16", row("wide", 0, K=16, wide_lanes=0), dict(WSEQ, KC=32)),
    ("wide, state a lane, K 17", row("wide", 0, K=17, wide_lanes=0), dict(WSEQ, KC=32)),
    ("wide, state a lane, K 32", row("wide", 0, K=32, wide_lanes=0), dict(WSEQ, KC=32)),
    ("wide, state a lane, K 33", row("wide", 0, K=33, wide_lanes=0), dict(WSEQ, KC=64)),
    ("wide, state a lane, K 64", row("wide", 0, K=64, wide_lanes=0), dict(WSEQ, KC=64)),
    # a chunk a lane, and what refuses it
    ("wide, hint 5000", row("wide", 5000), LANES),
    ("wide, hint 0", row("wide", 0), dict(LANES, room=1024)),
    ("wide, mixture", row("wide", 5000, mix=1), dict(WSEQ, mix=1)),
    ("wide, probed", row("wide", 5000, probes=1), WSEQ),
    ("wide, compat_chunks 7", row("wide", 5000, compat_chunks=7), dict(WSEQ, form="chunked", C=7)),
    ("wide, compat_chunks 1", row("wide", 5000, compat_chunks=1), WSEQ),
    ("wide, wide_lanes 0: 78 chunks", row("wide", 5000, wide_lanes=0), dict(WSEQ, form="chunked", C=78)),
    ("wide, compat_warmup 4", row("wide", 5000, compat_warmup=4), dict(LANES, W="4")),
    ("wide, compat_warmup -1", row("wide", 5000, compat_warmup=-1), dict(LANES, W="0")),
    # the bucket of the chunk-a-lane dispatch and the most chunks of a sweep
    ("wide K 2", row("wide", 5000, K=2), dict(LANES, KC=4)),
    ("wide K 16", row("wide", 5000, K=16), dict(LANES, KC=16)),
    ("wide K 17", row("wide", 5000, K=17), dict(LANES, KC=20)),
    ("wide K 32", row("wide", 5000, K=32), dict(LANES, KC=32)),
    ("wide K 33: padded to 36, two wavefronts", row("wide", 5000, K=33), dict(LANES, KC=36)),
    ("wide K 36", row("wide", 5000, K=36), dict(LANES, KC=36)),
    ("wide K 37: padded to 40, one wavefront", row("wide", 5000, K=37), dict(LANES, KC=40, max_chunks=65536)),
    ("wide K 40", row("wide", 5000, K=40), dict(LANES, KC=40, max_chunks=65536)),
    ("wide K 64", row("wide", 5000, K=64), dict(LANES, KC=64, max_chunks=65536)),
    ("wide_max_chunks 100", row("wide", 5000, wide_max_chunks=100), dict(LANES, max_chunks=100)),
    ("wide_max_chunks 100 at K 40", row("wide", 5000, K=40, wide_max_chunks=100), dict(LANES, KC=40, max_chunks=100)),
    ("wide_max_chunks 200000: clamped", row("wide", 5000, K=40, wide_max_chunks=200000), dict(LANES, KC=40, max_chunks=131072)),
    ("wide_lshift 5: chunks of 32", row("wide", 5000, wide_lshift=5), dict(LANES, min_L=32)),
    ("wide_lshift 0: chunks of 1", row("wide", 5000, wide_lshift=0), dict(LANES, min_L=1)),
    ("wide_w0 is the model's, not the plan's", row("wide", 5000, wide_w0=8), LANES),
    ("wide, hint 2^32 - 1: room beyond 32 bits", row("wide", 2 ** 32 - 1), dict(LANES, room=2 ** 32 - 1 + (2 ** 32 - 1) // 4 + 1024)),
]


def build(tmp_path, *flags):
    exe = str(tmp_path / ("rtk_plan" + "".join(flags).replace("=", "_").replace(",", "_")))
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *flags, "-I", os.path.join(REPO, "hammlet_amd", "csrc"), "-o", exe,
                    os.path.join(REPO, "tests", "fixtures", "rtk_plan_main.cpp")], check=True)
    return exe


def expected_line(p):
    return "%s %d %s %d %s %d %d %d | %d %d %d" % (p["form"], p["C"], p["W"], p["by_state"], p["exp"], p["KC"], p["pad"], p["mix"], p["max_chunks"], p["min_L"], p["room"])


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all")], ids=["plain", "sanitized"])
def test_rtk_plan_follows_the_rules(tmp_path, flags):
    """Every row's plan as the rules give it.  Built a second time with the address and undefined-behaviour sanitizers and run stand-alone."""
    exe = build(tmp_path, *flags)
    r = subprocess.run([exe], input="".join(c[1] + "\n" for c in CASES), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = r.stdout.splitlines()
    assert len(got) == len(CASES)
    for (name, _, want), line in zip(CASES, got):
        assert line == expected_line(want), name

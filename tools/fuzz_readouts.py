"""Randomised differential run of the recordings (tests/readout_fuzz_util.py): GPU against the CPU checker with several
recorders on at once, on random schemes and sweep paths.  Not part of the test suite; prints one line per configuration and
stops at the first difference.
    python tools/fuzz_readouts.py [--n 100] [--seed 1] [--only I] [many|wide|compat] [hostile]
--only I replays configuration I of the seed alone (what a failure of tests/test_gpu_readout_fuzz.py names)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hammlet_amd as hml

from tests.readout_fuzz_util import fuzz_readouts

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=100)
ap.add_argument("--seed", type=int, default=1)
ap.add_argument("--only", type=int, default=None)
ap.add_argument("modes", nargs="*", help="many | wide | compat, and hostile")
a = ap.parse_args()
if set(a.modes) - {"many", "wide", "compat", "hostile"}:
    ap.error("modes: many, wide, compat, hostile")
n = fuzz_readouts(hml, a.n, a.seed, many="many" in a.modes, wide="wide" in a.modes, compat="compat" in a.modes,
                  data="hostile" if "hostile" in a.modes else None, log=lambda s: print(s, flush=True), only=a.only)
print("all %d configurations identical" % (1 if a.only is not None else n))

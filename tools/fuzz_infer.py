"""Randomised differential run of the exact-inference passes (tests/infer_fuzz_util.py): GPU against the stand-alone restatements
on random data kinds, sizes, numbers of states, block regimes, parameters and geometries.  Not part of the test suite; prints one
line per configuration and stops at the first difference.
    python tools/fuzz_infer.py [--n 100] [--seed 1] [--only I]
--only I replays configuration I of the seed alone (what a failure of tests/test_gpu_infer_fuzz.py names)."""
import argparse
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hammlet_amd as hml

from tests.infer_fuzz_util import build_programs, fuzz_infer

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=100)
ap.add_argument("--seed", type=int, default=1)
ap.add_argument("--only", type=int, default=None)
a = ap.parse_args()
hml.load_library()
with tempfile.TemporaryDirectory() as d:
    n = fuzz_infer(hml, build_programs(d), a.n, a.seed, log=lambda s: print(s, flush=True), only=a.only)
print("all %d configurations identical" % n)

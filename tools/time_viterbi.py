"""Cost of a Viterbi decode (hml_viterbi): python tools/time_viterbi.py [case ...]      (profiles/viterbi_cost.txt)

Cases: c3      config 3's chain, 10^8 positions, 5 states, dynamic blocks (about 1.8 10^5 blocks)
       dense   10^7 positions, every position a block (weights x 10^9)
       depth   simulated read depth of config 5's kind, 2.5 10^7 positions
Per case: the chain runs 30 sweeps, then hml_viterbi (decode + run count, ending in a synchronise) is timed five times with the
host clock, with the numbers of hml_viterbi_info; next to it the time the sequential restatement for one host thread
(tests/fixtures/viterbi_ref_main.cpp over csrc/hml_viterbi_ref.h, g++ -O2) takes on the same blocks and parameters - tables and
recursion apart - and whether its path and score are the device's."""
import ctypes as C, os, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import bench, hammlet_amd
from tests import viterbi_util as vu

CASES = {
    "c3": ("c3_1e8_k5_dynamic", None, False),
    "dense": ("c2_1e7_k5", None, True),
    "depth": ("c5_2.5e8_depth_k5", 25_000_000, False),
}
program = vu.build_programs(tempfile.mkdtemp(), sanitized=False)["plain"]
for name in (sys.argv[1:] or list(CASES)):
    wl, T_override, every_position = CASES[name]
    T, K, levels, sigma, dwell, data_seed = bench.WORKLOADS[wl]
    T = T_override or T
    x = hammlet_amd.synth_depth(T, depth=dwell, ln_sigma=sigma, seed=data_seed, nthreads=8) if levels is None else hammlet_amd.synth_gauss(T, K, levels, sigma, dwell, data_seed, nthreads=8)
    g = hammlet_amd.Chain(device=0, seed=1)
    g.load(x)
    if every_position:
        g.scale_weights(1e9)
    g.set_model(K, g.autoprior(0.2, 0.9))
    g.sample_prior()
    g.iterate("F", 30, 0)
    g.sync()
    B = g.num_blocks()
    print("%s: T=%d K=%d blocks=%d" % (name, T, K, B), flush=True)
    for label, options in (("defaults", {}), ("W=256", {"viterbi_W": 256}), ("W=1024 L=256", {"viterbi_W": 1024, "viterbi_L": 256})):
        for k in ("viterbi_W", "viterbi_L"):
            g.set_option(k, options.get(k, 0))
        times = []
        n, fixed = C.c_uint64(), C.c_int64()
        for rep in range(5):
            t0 = time.perf_counter()
            hammlet_amd.capi._check(g.lib.hml_viterbi(g.h, C.byref(n), None, None, C.byref(fixed), None))
            times.append(1e3 * (time.perf_counter() - t0))
        print("  %-13s hml_viterbi: %s ms   runs %d score_fixed %d   %s" % (label, " ".join("%.2f" % t for t in times), n.value, fixed.value, g.viterbi_info()), flush=True)
    q = g.viterbi_states()
    t0 = time.perf_counter()
    want = vu.run_case(program, vu.chain_case(g), want_emit=False)
    print("  sequential restatement, one core: tables %.1f ms, recursion + back-track %.1f ms (the program with its text input and output: %.1f s); path %s, score %s"
          % (1e3 * want["seconds"][0], 1e3 * want["seconds"][1], time.perf_counter() - t0, "equal" if np.array_equal(q, want["path"]) else "DIFFERENT",
             "equal" if want["score"] == fixed.value else "DIFFERENT"), flush=True)
    g.close()
    del x

"""Cost of the smoothing read-out (hml_posterior): python tools/time_posterior.py [case ...]      (profiles/posterior_cost.txt)

Cases: c3      config 3's chain, 10^8 positions, 5 states, dynamic blocks (about 1.8 10^5 blocks)
       dense   10^7 positions, every position a block (weights x 10^9)
       depth   simulated read depth of config 5's kind, 2.5 10^7 positions
Per case: the chain runs 30 sweeps, then hml_posterior without gamma (both recursions, the combining pass and the tree sum,
ending in a synchronise) is timed five times with the host clock, with the numbers of hml_posterior_info; next to it the time
the sequential restatement for one host thread (tests/fixtures/posterior_ref_main.cpp over csrc/hml_posterior_ref.h, g++ -O2)
takes on the same blocks and parameters - tables and smoothing apart - and whether its log-likelihood and runs are the device's."""
import ctypes as C, os, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import bench, hammlet_amd
from tests import posterior_util as pu

CASES = {
    "c3": ("c3_1e8_k5_dynamic", None, False),
    "dense": ("c2_1e7_k5", None, True),
    "depth": ("c5_2.5e8_depth_k5", 25_000_000, False),
}
program = pu.build_programs(tempfile.mkdtemp(), sanitized=False)["plain"]
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
    loglik, degenerate = C.c_double(), C.c_uint64()
    for label, options in (("defaults", {}), ("W=64", {"posterior_W": 64}), ("W=1024 L=256", {"posterior_W": 1024, "posterior_L": 256})):
        for k in ("posterior_W", "posterior_L"):
            g.set_option(k, options.get(k, 0))
        times = []
        for rep in range(5):
            t0 = time.perf_counter()
            hammlet_amd.capi._check(g.lib.hml_posterior(g.h, None, C.byref(loglik), C.byref(degenerate)))
            times.append(1e3 * (time.perf_counter() - t0))
        print("  %-13s hml_posterior: %s ms   loglik %.17g degenerate %d   %s" % (label, " ".join("%.2f" % t for t in times), loglik.value, degenerate.value, g.posterior_info()),
              flush=True)
    run_len, run_state, run_conf = g.posterior_rle()
    t0 = time.perf_counter()
    want = pu.run_case(program, pu.chain_case(g), want_rows=False)
    same_runs = np.array_equal(run_len, want["run_len"].astype(np.uint64)) and np.array_equal(run_state, want["run_state"]) and np.array_equal(pu.words(run_conf), want["run_conf"])
    print("  sequential restatement, one core: tables %.1f ms, smoothing %.1f ms (the program with its text input and output: %.1f s); log-likelihood %s, runs %s (%d)"
          % (1e3 * want["seconds"][0], 1e3 * want["seconds"][1], time.perf_counter() - t0, "equal" if pu.words([loglik.value])[0] == want["loglik"][0] else "DIFFERENT",
             "equal" if same_runs else "DIFFERENT", len(run_len)), flush=True)
    g.close()
    del x

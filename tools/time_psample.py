"""Cost of the path sampler (hml_posterior_sample): python tools/time_psample.py [case ...]      (profiles/psample_cost.txt)

Cases: c3      config 3's chain, 10^8 positions, 5 states, dynamic blocks (about 1.8 10^5 blocks)
       dense   10^7 positions, every position a block (weights x 10^9)
       depth   simulated read depth of config 5's kind, 2.5 10^7 positions
Per case: the chain runs 30 sweeps; hml_posterior alone (no gamma) is timed five times; then hml_posterior_sample with segments
and scores (no paths) for 64, 1024 and 4096 draws at the default geometry, and 1024 draws under other geometries, five times each
with the host clock around the call, with the numbers of hml_posterior_sample_info; next to it the time the sequential
restatement for one host thread (tests/fixtures/sample_ref_main.cpp over csrc/hml_sample_ref.h, g++ -O2) takes for 64 draws (8 beyond 10^6 blocks) on
the same blocks and parameters - the forward rows and the draws apart - and whether its segments and scores are the device's."""
import ctypes as C, os, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import bench, hammlet_amd
from tests import sample_util as su

CASES = {
    "c3": ("c3_1e8_k5_dynamic", None, False),
    "dense": ("c2_1e7_k5", None, True),
    "depth": ("c5_2.5e8_depth_k5", 25_000_000, False),
}
GEOMETRIES = (("L=64", {"sample_L": 64}), ("W=64", {"sample_W": 64}), ("W=16", {"sample_W": 16}), ("L=1024", {"sample_L": 1024}),
              ("L=1024 W=64", {"sample_L": 1024, "sample_W": 64}))
program = su.build_programs(tempfile.mkdtemp(), sanitized=False)["plain"]


def timed(g, count, seed=1):
    seg, score, bad = np.empty(count, np.uint64), np.empty(count, np.int64), C.c_uint64()
    times = []
    for rep in range(5):
        t0 = time.perf_counter()
        hammlet_amd.capi._check(g.lib.hml_posterior_sample(g.h, 0, count, seed, None, seg.ctypes.data, score.ctypes.data, None, None, C.byref(bad)))
        times.append(1e3 * (time.perf_counter() - t0))
    return times, seg, score, bad.value


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
    times = []
    for rep in range(5):
        t0 = time.perf_counter()
        hammlet_amd.capi._check(g.lib.hml_posterior(g.h, None, C.byref(loglik), C.byref(degenerate)))
        times.append(1e3 * (time.perf_counter() - t0))
    print("  hml_posterior alone: %s ms" % " ".join("%.2f" % t for t in times), flush=True)
    first = None
    for count in (64, 1024, 4096):
        times, seg, score, bad = timed(g, count)
        if first is None:
            first = (seg.copy(), score.copy())
        print("  %5d draws  defaults     : %s ms   degenerate %d   %s" % (count, " ".join("%.2f" % t for t in times), bad, g.posterior_sample_info()), flush=True)
    for label, options in GEOMETRIES:
        for k in ("sample_W", "sample_L"):
            g.set_option(k, options.get(k, 0))
        times, seg, score, bad = timed(g, 1024)
        same = np.array_equal(seg[:64], first[0]) and np.array_equal(score[:64], first[1])
        print("   1024 draws  %-13s: %s ms   %s   first 64 draws %s" % (label, " ".join("%.2f" % t for t in times), g.posterior_sample_info(), "equal" if same else "DIFFERENT"), flush=True)
    for k in ("sample_W", "sample_L"):
        g.set_option(k, 0)
    t0 = time.perf_counter()
    n_ref = 64 if B < 1000000 else 8      # (a draw takes the core about a second per 10^7 blocks)
    want = su.run_program(program, su.chain_case(g), 0, n_ref, 1, mode="timing")
    same = np.array_equal(want["segments"].astype(np.uint64), first[0][:n_ref]) and np.array_equal(want["score_fixed"], first[1][:n_ref])
    print("  sequential restatement, one core, %d draws: tables, forward rows and decode %.1f ms, the draws %.1f ms (the program with its text input and output: %.1f s); "
          "segments and scores %s" % (n_ref, 1e3 * want["seconds"][0], 1e3 * want["seconds"][1], time.perf_counter() - t0, "equal" if same else "DIFFERENT"), flush=True)
    g.close()
    del x

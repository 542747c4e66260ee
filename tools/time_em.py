"""Cost of the E-step and of an EM step (hml_expected_counts, hml_em_step): python tools/time_em.py [case ...]      (profiles/em_cost.txt)

Cases: the three of tools/time_posterior.py
       c3      config 3's chain, 10^8 positions, 5 states, dynamic blocks (about 1.8 10^5 blocks)
       dense   10^7 positions, every position a block (weights x 10^9)
       depth   simulated read depth of config 5's kind, 2.5 10^7 positions
Per case: the chain runs 30 sweeps, then hml_posterior without gamma, hml_expected_counts and hml_em_step (maximum likelihood;
the parameters are put back before each) are each timed five times with the host clock.  The new pass is what hml_expected_counts
takes beyond hml_posterior; its traffic is counted as the rows alpha and beta read once (16 B K bytes), X written and read
(16 B; only above 16 states, below that X never leaves the workgroup), a block's start and integral-array entries
(4 + 16 D bytes a block) and the level-1 partials written (8 ncols B / 64).
Next to it: the time the sequential restatement for one host thread (tests/fixtures/em_ref_main.cpp over csrc/hml_em_ref.h,
g++ -O2) takes for the same E-step, and whether its words are the device's."""
import ctypes as C, os, statistics, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import bench, hammlet_amd
from tests import em_util as eu
from tests import posterior_util as pu

CASES = {
    "c3": ("c3_1e8_k5_dynamic", None, False),
    "dense": ("c2_1e7_k5", None, True),
    "depth": ("c5_2.5e8_depth_k5", 25_000_000, False),
}


def five(call, before=None):
    times = []
    for rep in range(5):
        if before:
            before()
        t0 = time.perf_counter()
        call()
        times.append(1e3 * (time.perf_counter() - t0))
    return times


program = eu.build_programs(tempfile.mkdtemp(), sanitized=False)["plain"]
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
    B, D = g.num_blocks(), g.D
    ncols = K * K + K * (2 + 2 * D)
    print("%s: T=%d K=%d blocks=%d columns=%d" % (name, T, K, B, ncols), flush=True)
    mv, (A, pi) = g.theta(), g.transitions()
    loglik, degenerate = C.c_double(), C.c_uint64()
    t_post = five(lambda: hammlet_amd.capi._check(g.lib.hml_posterior(g.h, None, C.byref(loglik), C.byref(degenerate))))
    t_cnt = five(g.expected_counts)
    t_step = five(g.em_step, before=lambda: g.set_parameters(mv, A, pi))
    g.set_parameters(mv, A, pi)
    for label, t in (("hml_posterior", t_post), ("hml_expected_counts", t_cnt), ("hml_em_step", t_step)):
        print("  %-20s %s ms   median %.2f" % (label, " ".join("%.2f" % v for v in t), statistics.median(t)), flush=True)
    extra = statistics.median(t_cnt) - statistics.median(t_post)
    traffic = 16.0 * B * K + (16.0 * B if K > 16 else 0.0) + (4 + 16 * D) * B + 8.0 * ncols * ((B + 63) // 64)
    print("  the new pass: %.2f ms beyond hml_posterior, %.1f MB counted, %.1f GB/s" % (extra, traffic / 1e6, traffic / 1e9 / max(extra, 1e-6) * 1e3), flush=True)
    got = eu.chain_counts_words(g.expected_counts())
    t0 = time.perf_counter()
    want = eu.run_program(program, "estep", pu.chain_case(g))
    same = all(np.array_equal(got[k], want[k]) for k in eu.COUNT_KEYS + ("loglik",)) and got["degenerate"] == want["degenerate"] and got["xi_degenerate"] == want["xi_degenerate"]
    print("  sequential restatement, one core: E-step %.1f ms (the program with its text input and output: %.1f s); words %s"
          % (1e3 * want["seconds"], time.perf_counter() - t0, "equal" if same else "DIFFERENT"), flush=True)
    g.close()
    del x

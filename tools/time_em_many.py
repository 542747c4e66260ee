"""Cost of EM from many starts (hml_em_fit_many) against the same fits run one after the other:
    python tools/time_em_many.py batch|sequential [case ...]                                        (profiles/em_many_cost.txt)

Cases: c3      config 3's chain, 10^8 positions, 5 states, dynamic blocks (about 1.8 10^5 blocks)
       dense   10^7 positions, every position a block (weights x 10^9)
Per case: the chain runs 30 sweeps; R = 16 starts come from the generator's Python restatement (tests/em_many_util.py - the
words of hml_em_starts, and available to a build without it); 10 steps at a tolerance no step can meet, so that every member
runs every step.  Timed five times with the host clock, the parameters put back before each:
    batch        one hml_em_fit_many over the 16 starts (not installed), and one single hml_em_fit from start 0 beside it
    sequential   the 16 fits as hml_set_parameters + hml_em_fit, one after the other - what a caller did before; this mode uses
                 nothing the batch added, so it runs in the parent commit's tree on the parent's library: the yardstick.  Run
                 the two modes in separate processes, alternating.
Both print a digest of all members' final floats: equal digests, equal fits."""
import hashlib, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import bench, hammlet_amd
from tests import em_many_util as mu

CASES = {"c3": ("c3_1e8_k5_dynamic", False), "dense": ("c2_1e7_k5", True)}
R, STEPS, TOL, SEED = 16, 10, -1.0, 1

mode = sys.argv[1]
assert mode in ("batch", "sequential"), __doc__
for name in (sys.argv[2:] or list(CASES)):
    wl, every_position = CASES[name]
    T, K, levels, sigma, dwell, data_seed = bench.WORKLOADS[wl]
    x = hammlet_amd.synth_gauss(T, K, levels, sigma, dwell, data_seed, nthreads=8)
    g = hammlet_amd.Chain(device=0, seed=1)
    g.load(x)
    if every_position:
        g.scale_weights(1e9)
    g.set_model(K, g.autoprior(0.2, 0.9))
    g.sample_prior()
    g.iterate("F", 30, 0)
    g.sync()
    mv, (A, pi) = g.theta(), g.transitions()
    starts = mu.starts(K, K, R, SEED, 1.0, mv, A, pi)
    print("%s %s: T=%d K=%d blocks=%d members=%d steps=%d" % (mode, name, T, K, g.num_blocks(), R, STEPS), flush=True)
    digest = hashlib.sha256()
    times, single = [], []
    for rep in range(5):
        g.set_parameters(mv, A, pi)
        if mode == "batch":
            t0 = time.perf_counter()
            got = g.em_fit_many(starts=starts, max_steps=STEPS, rel_tol=TOL, install=False)
            times.append(1e3 * (time.perf_counter() - t0))
            final = [got["mean_var"].tobytes(), got["A"].tobytes(), got["pi"].tobytes(), got["trace"].tobytes()]
            t0 = time.perf_counter()
            g.em_fit(STEPS, rel_tol=TOL)
            single.append(1e3 * (time.perf_counter() - t0))
        else:
            final = [[], [], [], []]
            t0 = time.perf_counter()
            for r in range(R):
                g.set_parameters(starts[0][r], starts[1][r], starts[2][r])
                trace = g.em_fit(STEPS, rel_tol=TOL)[0]
                fA, fpi = g.transitions()
                for part, v in zip(final, (g.theta(), fA, fpi, trace)):
                    part.append(v.tobytes())
            times.append(1e3 * (time.perf_counter() - t0))
            final = [b"".join(part) for part in final]
        if rep == 0:
            for part in final:
                digest.update(part)
    print("  %-28s %s ms   median %.1f   spread %.1f" % ("16 fits, " + mode, " ".join("%.1f" % v for v in times), statistics.median(times), max(times) - min(times)), flush=True)
    if single:
        print("  %-28s %s ms   median %.1f" % ("one hml_em_fit", " ".join("%.1f" % v for v in single), statistics.median(single)), flush=True)
        print("  info: %s" % g.em_many_info(), flush=True)
    print("  digest of the fits: %s" % digest.hexdigest()[:16], flush=True)
    g.close()
    del x

"""What the chain's history costs: plain sweeps (no event brackets) of the bench workload with the history off, on for every
sweep and on for every tenth, on fresh chains over one trace in one process:
    python tools/time_history.py [workload] [sweeps] [every ...]     (every = 0: off; default 0 1 10)
One line per setting: ms per sweep by the host clock, the rows written, the rows dropped."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
import hammlet_amd  # noqa: E402

wl = sys.argv[1] if len(sys.argv) > 1 else "c3_1e8_k5_dynamic"
n = int(sys.argv[2]) if len(sys.argv) > 2 else 2000
settings = [int(a) for a in sys.argv[3:]] or [0, 1, 10]
T, K, levels, sigma, dwell, data_seed = bench.WORKLOADS[wl]
x = hammlet_amd.synth_depth(T, depth=dwell, ln_sigma=sigma, seed=data_seed, nthreads=8) if levels is None else hammlet_amd.synth_gauss(T, K, levels, sigma, dwell, data_seed, nthreads=8)
for every in settings:
    ch = hammlet_amd.Chain(device=0, seed=1)
    ch.load(x)
    ch.set_model(K, ch.autoprior(0.2, 0.9))
    ch.sample_prior()
    ch.set_recording(marginals=False)
    if every:
        ch.set_history(True, every)
    ch.iterate("F", 40, 0)
    ch.sync()
    t0 = time.perf_counter()
    ch.iterate("F", n, 0)
    ch.sync()
    t1 = time.perf_counter()
    rows = ch.history()
    print("%s history %s: %.4f ms/sweep over %d sweeps, %d rows, %d dropped, B %d%s" % (
          wl, "every %d" % every if every else "off", 1e3 * (t1 - t0) / n, n, len(rows), ch.history_dropped(), ch.num_blocks(),
          ", last loglik %.17g" % (rows[-1, 2] + rows[-1, 3]) if len(rows) else ""))
    ch.close()

"""Cost of the regions recording: python tools/time_regions.py [workload | c3u] [sweeps]

Times `F n 10` (every tenth sweep recorded) with the marginals alone ("off") and with 20 000 regions of 5 000 positions and the
edges -0.5 0.5 on, three runs each, then the per-kernel times of the recording from hml_profile_get over 20 recorded sweeps.
c3u: the config-3 trace with the breakpoint weights times 1e9 - every position a block, the weakly compressed geometry (fewer
sweeps by default).  A tree without the regions calls runs the "off" leg only: copy this file into it to compare two commits."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import bench, hammlet_amd
args = [a for a in sys.argv[1:] if not a.startswith("--")]
wl = args[0] if len(args) > 0 else "c3_1e8_k5_dynamic"
dense = wl == "c3u"
n = int(args[1]) if len(args) > 1 else (40 if dense else 400)
T, K, levels, sigma, dwell, data_seed = bench.WORKLOADS["c3_1e8_k5_dynamic" if dense else wl]
x = hammlet_amd.synth_depth(T, depth=dwell, ln_sigma=sigma, seed=data_seed, nthreads=8) if levels is None else hammlet_amd.synth_gauss(T, K, levels, sigma, dwell, data_seed, nthreads=8)
has_regions = hasattr(hammlet_amd.Chain, "set_regions")
EDGES = (-0.5, 0.5)
R, LENGTH = 20000, 5000
start = np.random.RandomState(1).randint(0, T - LENGTH + 1, size=R).astype(np.uint32)
FAMILIES = ("regions", "regions_chunks", "regions_scan", "regions_accumulate", "marginals", "params")


def leg(name, regions):
    ch = hammlet_amd.Chain(device=0, seed=1)
    ch.load(x)
    if dense:
        ch.scale_weights(1e9)
    ch.set_model(K, ch.autoprior(0.2, 0.9))
    ch.sample_prior()
    if regions:
        ch.set_regions(start, start + LENGTH, EDGES)
    ch.iterate("F", 70 if dense else 40, 10); ch.sync()
    times = []
    for rep in range(3):
        t0 = time.perf_counter(); ch.iterate("F", n, 10); ch.sync(); t1 = time.perf_counter()
        times.append(1e3 * (t1 - t0) / n)
    print("%s %s: %s ms/sweep (three runs of %d sweeps, every tenth recorded; %.3e blocks)" % (wl, name, " ".join("%.4f" % t for t in times), n, ch.num_blocks()), flush=True)
    if regions:
        ch.profile_enable(2)
        ch.iterate("F", 200, 10); ch.sync()
        for fam in FAMILIES:
            ms, launches = ch.profile_get(fam)
            print("  %-20s %8.2f us per recorded sweep (%d brackets)" % (fam, 1e3 * ms / max(1, launches), launches), flush=True)
        ch.profile_enable(0)
        got = ch.regions()
        print("  N = %d, regions whole in every sweep %d, in none %d" % (got["N"], int(np.sum(got["whole"] == got["N"])), int(np.sum(got["whole"] == 0))), flush=True)
    ch.close()


leg("regions off", False)
if has_regions:
    leg("regions on (%d regions of %d positions, edges %s)" % (R, LENGTH, " ".join(str(e) for e in EDGES)), True)

"""Cost of break recording on the bench workload: python tools/time_breaks.py [workload] [sweeps] [--readouts]

Times `F n 10` (every tenth sweep recorded) with the marginals alone, with break recording on, and with breaks and
levels on; with --readouts also one call each of breaks_list, breaks_consensus and breaks_dense on the chain that
recorded.  Set HML_LIBRARY to time another build's first leg (a build without the break calls runs that leg only)."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench, hammlet_amd
args = [a for a in sys.argv[1:] if not a.startswith("--")]
wl = args[0] if len(args) > 0 else "c3_1e8_k5_dynamic"
n = int(args[1]) if len(args) > 1 else 400
T, K, levels, sigma, dwell, data_seed = bench.WORKLOADS[wl]
x = hammlet_amd.synth_depth(T, depth=dwell, ln_sigma=sigma, seed=data_seed, nthreads=8) if levels is None else hammlet_amd.synth_gauss(T, K, levels, sigma, dwell, data_seed, nthreads=8)
has_breaks = hasattr(hammlet_amd.Chain, "set_break_recording")


def leg(name, breaks, lev):
    ch = hammlet_amd.Chain(device=0, seed=1)
    ch.load(x)
    ch.set_model(K, ch.autoprior(0.2, 0.9))
    ch.sample_prior()
    if breaks:
        ch.set_break_recording(True)
    if lev:
        ch.set_level_recording(True)
    ch.iterate("F", 40, 10); ch.sync()
    times = []
    for rep in range(3):
        t0 = time.perf_counter(); ch.iterate("F", n, 10); ch.sync(); t1 = time.perf_counter()
        times.append(1e3 * (t1 - t0) / n)
    print("%s %s: %s ms/sweep (three runs of %d sweeps, every tenth recorded)" % (wl, name, " ".join("%.4f" % t for t in times), n), flush=True)
    return ch


leg("marginals only", False, False).close()
if has_breaks:
    ch = leg("breaks on", True, False)
    if "--readouts" in sys.argv:
        import torch
        out = torch.empty(T, dtype=torch.float32, device="cuda:0")
        M, N = len(ch.breaks_list()[0]), ch.breaks_list()[2]
        for name, call in (("breaks_list", ch.breaks_list), ("breaks_consensus(16, N/2)", lambda: ch.breaks_consensus(16, max(1, N // 2))),
                           ("breaks_dense(16)", lambda: (ch.breaks_dense(out.data_ptr(), 16), torch.cuda.synchronize()))):
            t0 = time.perf_counter(); r = call(); t1 = time.perf_counter()
            print("T=%d %s: %.2f ms (%d breakpoints listed)" % (T, name, 1e3 * (t1 - t0), M), flush=True)
    ch.close()
    leg("breaks and levels on", True, True).close()

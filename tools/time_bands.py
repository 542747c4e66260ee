"""Cost of band recording on the bench workload: python tools/time_bands.py [workload] [sweeps] [--readouts]

Times `F n 10` (every tenth sweep recorded) with the marginals alone and with the level bands on (edges -0.5 0.5); with
--readouts also one call each of bands_rle, bands_call (most probable band, median) and bands_dense_device, plain and
cumulative, on the chain that recorded.  Set HML_LIBRARY to time another build's first leg (a build without the band calls
runs that leg only)."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench, hammlet_amd
args = [a for a in sys.argv[1:] if not a.startswith("--")]
wl = args[0] if len(args) > 0 else "c3_1e8_k5_dynamic"
n = int(args[1]) if len(args) > 1 else 400
T, K, levels, sigma, dwell, data_seed = bench.WORKLOADS[wl]
x = hammlet_amd.synth_depth(T, depth=dwell, ln_sigma=sigma, seed=data_seed, nthreads=8) if levels is None else hammlet_amd.synth_gauss(T, K, levels, sigma, dwell, data_seed, nthreads=8)
has_bands = hasattr(hammlet_amd.Chain, "set_level_bands")
EDGES = (-0.5, 0.5)


def leg(name, bands):
    ch = hammlet_amd.Chain(device=0, seed=1)
    ch.load(x)
    ch.set_model(K, ch.autoprior(0.2, 0.9))
    ch.sample_prior()
    if bands:
        ch.set_level_bands(EDGES)
    ch.iterate("F", 40, 10); ch.sync()
    times = []
    for rep in range(3):
        t0 = time.perf_counter(); ch.iterate("F", n, 10); ch.sync(); t1 = time.perf_counter()
        times.append(1e3 * (t1 - t0) / n)
    print("%s %s: %s ms/sweep (three runs of %d sweeps, every tenth recorded)" % (wl, name, " ".join("%.4f" % t for t in times), n), flush=True)
    return ch


leg("marginals only", False).close()
if has_bands:
    ch = leg("bands on", True)
    if "--readouts" in sys.argv:
        import torch
        out = torch.empty((len(EDGES) + 1, T), dtype=torch.int32, device="cuda:0")
        seg, cnt, N = ch.bands_rle()
        for name, call in (("bands_rle", ch.bands_rle), ("bands_call(0)", lambda: ch.bands_call(0)), ("bands_call(median)", lambda: ch.bands_call((N + 1) // 2)),
                           ("bands_dense_device", lambda: (ch.bands_dense_device(out.data_ptr()), torch.cuda.synchronize())),
                           ("bands_dense_device cumulative", lambda: (ch.bands_dense_device(out.data_ptr(), True), torch.cuda.synchronize()))):
            t0 = time.perf_counter(); r = call(); t1 = time.perf_counter()
            print("T=%d %s: %.2f ms (%d band segments, N = %d)" % (T, name, 1e3 * (t1 - t0), len(seg), N), flush=True)
    ch.close()

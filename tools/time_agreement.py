"""Cost of the agreement read-outs on the bench workload: python tools/time_agreement.py [workload] [sweeps] [chains]

Eight chains attached to one trace run `F n 10` (every tenth sweep recorded) with the level recording on; then one call each of
levels_agreement_rle, levels_agreement_summary and levels_agreement_dense_device over the eight contexts, beside the summed
time of the eight chains' own levels_rle calls on the same contexts - the cost of fetching the same inputs one chain at a time.
Every read-out is timed three times (the first call of a kind loads its kernels)."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench, hammlet_amd
args = [a for a in sys.argv[1:] if not a.startswith("--")]
wl = args[0] if len(args) > 0 else "c3_1e8_k5_dynamic"
n = int(args[1]) if len(args) > 1 else 100
n_chains = int(args[2]) if len(args) > 2 else 8
T, K, levels, sigma, dwell, data_seed = bench.WORKLOADS[wl]
x = hammlet_amd.synth_depth(T, depth=dwell, ln_sigma=sigma, seed=data_seed, nthreads=8) if levels is None else hammlet_amd.synth_gauss(T, K, levels, sigma, dwell, data_seed, nthreads=8)

chains = []
for k in range(n_chains):
    ch = hammlet_amd.Chain(device=0, seed=1, chain_id=k)
    if k == 0:
        ch.load(x)
    else:
        ch.attach(chains[0])
    ch.set_model(K, ch.autoprior(0.2, 0.9))
    ch.set_level_recording(True)
    ch.sample_prior()
    chains.append(ch)
hammlet_amd.iterate_many(chains, "F", n, 10)
for ch in chains:
    ch.sync()

import torch
out = torch.empty((chains[0].D, T), dtype=torch.float32, device="cuda:0")


def timed(call):
    times = []
    for rep in range(3):
        t0 = time.perf_counter(); r = call(); torch.cuda.synchronize(); t1 = time.perf_counter()
        times.append(1e3 * (t1 - t0))
    return r, " ".join("%.2f" % t for t in times)


rles, t = timed(lambda: [ch.levels_rle() for ch in chains])
print("T=%d, %d chains, N = %d: levels_rle of every chain, summed: %s ms (%s segments)" % (T, n_chains, rles[0][1], t, " ".join(str(len(r[0])) for r in rles)), flush=True)
(seg, N, within, between, rhat), t = timed(lambda: hammlet_amd.levels_agreement_rle(chains))
print("levels_agreement_rle: %s ms (%d union segments)" % (t, len(seg)), flush=True)
(above, largest, infinite), t = timed(lambda: hammlet_amd.levels_agreement_summary(chains, 1.1))
print("levels_agreement_summary(1.1): %s ms (%d positions above 1.1, %d infinite, largest finite %.4g)" % (t, int(above[0]), int(infinite[0]), largest[0]), flush=True)
_, t = timed(lambda: hammlet_amd.levels_agreement_dense_device(chains, out.data_ptr()))
print("levels_agreement_dense_device: %s ms" % t, flush=True)
for ch in chains:
    ch.close()

"""Cost of the sparse payloads on the bench workload: python tools/time_recording_payload.py [workload] [sweeps] [chains]

Eight chains attached to one trace run `F n 10` (every tenth sweep recorded) with the levels, breakpoints and bands recorded;
then, per kind, chain 1's recording goes into contexts that recorded nothing: hml_recording_payload_size + hml_recording_export,
hml_recording_merge_payload of the exported bytes, hml_recording_merge_across on the one device, and beside them the existing
same-device hml_levels_merge / hml_breaks_merge / hml_bands_merge of the same chain - the yardstick.  Every call is timed three
times with the host clock (each ends in a synchronise; the first call of a kind loads its kernels and, for a destination,
allocates and zeroes its recorder).  The copy between two GPUs is not in these numbers: it needs a box with two."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench, hammlet_amd
args = [a for a in sys.argv[1:] if not a.startswith("--")]
wl = args[0] if len(args) > 0 else "c3_1e8_k5_dynamic"
n = int(args[1]) if len(args) > 1 else 100
n_chains = int(args[2]) if len(args) > 2 else 8
T, K, levels, sigma, dwell, data_seed = bench.WORKLOADS[wl]
x = hammlet_amd.synth_depth(T, depth=dwell, ln_sigma=sigma, seed=data_seed, nthreads=8) if levels is None else hammlet_amd.synth_gauss(T, K, levels, sigma, dwell, data_seed, nthreads=8)
EDGES = [-0.5, 0.5]


def attached(k, record):
    ch = hammlet_amd.Chain(device=0, seed=1, chain_id=k)
    if k == 0:
        ch.load(x)
    else:
        ch.attach(chains[0])
    ch.set_model(K, ch.autoprior(0.2, 0.9))
    if record:
        ch.set_level_recording(True)
        ch.set_break_recording(True)
        ch.set_level_bands(EDGES)
    ch.sample_prior()
    return ch


chains = []
for k in range(n_chains):
    chains.append(attached(k, True))
hammlet_amd.iterate_many(chains, "F", n, 10)
for ch in chains:
    ch.sync()

import torch


def timed(call):
    times = []
    for rep in range(3):
        t0 = time.perf_counter(); r = call(); torch.cuda.synchronize(); t1 = time.perf_counter()
        times.append(1e3 * (t1 - t0))
    return r, " ".join("%.2f" % t for t in times)


src = chains[1]
sinks = [attached(100 + j, False) for j in range(3)]   # destinations of merge_payload, merge_across and the existing merge
print("T=%d, %d chains, %d recorded sweeps each; one MI355X, every context on it" % (T, n_chains, n // 10), flush=True)
for kind, name, existing in ((hammlet_amd.RECORDING_LEVELS, "levels", lambda d, s: d.merge_levels(s)),
                             (hammlet_amd.RECORDING_BREAKS, "breaks", lambda d, s: d.breaks_merge(s)),
                             (hammlet_amd.RECORDING_BANDS, "bands", lambda d, s: d.merge_bands(s))):
    size = src.recording_payload_size(kind)
    buf = torch.zeros(size, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    _, t_export = timed(lambda: src.recording_export(kind, buf.data_ptr(), src.recording_payload_size(kind)))
    M = int(buf[32:40].cpu().numpy().view("<u8")[0])
    _, t_merge = timed(lambda: sinks[0].recording_merge_payload(kind, buf.data_ptr(), size))
    _, t_across = timed(lambda: sinks[1].recording_merge_across(src, kind))
    _, t_existing = timed(lambda: existing(sinks[2], src))
    print("%s: M = %d, payload %d bytes (dense rows: %d bytes)" % (name, M, size, {0: 16, 1: 4, 2: 12}[kind] * (T + 1)), flush=True)
    print("  payload_size + export:        %s ms" % t_export, flush=True)
    print("  merge_payload:                %s ms" % t_merge, flush=True)
    print("  merge_across (one device):    %s ms" % t_across, flush=True)
    print("  existing same-device merge:   %s ms" % t_existing, flush=True)
for ch in chains + sinks:
    ch.close()

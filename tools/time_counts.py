"""Cost of the count read-outs of the smoothing (hml_posterior_region_counts):
python tools/time_counts.py      (profiles/counts_cost.txt)

The case is config 3's chain: 10^8 positions, 5 states, dynamic blocks (about 1.8 10^5 blocks).  The chain runs 30 sweeps, then
each call is timed five times with the host clock, in one process:
  hml_posterior without gamma - the yardstick: the smoothing pass every exact read-out follows, in the same build;
  hml_posterior_region_counts with 20 000 random regions (the regions of tools/time_pairs.py: a geometric number of positions,
  10^5 on average) at max_breaks = 8, and with one region over the whole trace - a single serial chain of B - 1 steps;
  hml_posterior_regions on the same 20 000 regions;
  hml_posterior_sample_regions with 4096 draws on the same 20 000 regions, max_breaks = 8.
The walks' own time is what a call takes beyond hml_posterior; it is set against the steps hml_posterior_counts_info reports.
The lines are printed and written into profiles/counts_cost.txt between the two marker lines "## tools/time_counts.py: begin" and
"## tools/time_counts.py: end" (the file is created with them if it is not there); what stands outside the markers is written by
hand and kept."""
import ctypes as C, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import bench, hammlet_amd

WORKLOAD = "c3_1e8_k5_dynamic"
N_REGIONS, H, DRAWS = 20000, 8, 4096
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "counts_cost.txt")
BEGIN, END = "## tools/time_counts.py: begin", "## tools/time_counts.py: end"
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def write_out():
    """the lines between the markers of OUT, everything else kept"""
    old = open(OUT).read().split("\n") if os.path.exists(OUT) else []
    if BEGIN in old and END in old and old.index(BEGIN) < old.index(END):
        new = old[:old.index(BEGIN) + 1] + lines + old[old.index(END):]
    else:
        new = old + [BEGIN] + lines + [END, ""]
    with open(OUT, "w") as f:
        f.write("\n".join(new))


def five(call):
    times = []
    for rep in range(5):
        t0 = time.perf_counter()
        call()
        times.append(1e3 * (time.perf_counter() - t0))
    return times


T, K, levels, sigma, dwell, data_seed = bench.WORKLOADS[WORKLOAD]
x = hammlet_amd.synth_gauss(T, K, levels, sigma, dwell, data_seed, nthreads=8)
g = hammlet_amd.Chain(device=0, seed=1)
g.load(x)
g.set_model(K, g.autoprior(0.2, 0.9))
g.sample_prior()
g.iterate("F", 30, 0)
g.sync()
B = g.num_blocks()
say("c3: T=%d K=%d blocks=%d regions=%d max_breaks=%d draws=%d" % (T, K, B, N_REGIONS, H, DRAWS))
rng = np.random.default_rng(1)
start = rng.integers(0, T, N_REGIONS).astype(np.uint32)
end = np.minimum(start.astype(np.int64) + rng.geometric(1e-5, N_REGIONS), T).astype(np.uint32)
whole_start, whole_end = np.array([0], np.uint32), np.array([T], np.uint32)
loglik, degenerate, bad = C.c_double(), C.c_uint64(), C.c_uint64()
hist, ws, av = np.empty((N_REGIONS, H + 1)), np.empty((N_REGIONS, K)), np.empty((N_REGIONS, K))
whole, eb, share = np.empty(N_REGIONS), np.empty(N_REGIONS), np.empty((N_REGIONS, K))
s_hist, s_ws = np.empty((N_REGIONS, H + 1), np.uint32), np.empty((N_REGIONS, K), np.uint32)
s_sum, s_sq = np.empty(N_REGIONS, np.uint64), np.empty(N_REGIONS, np.uint64)
check = hammlet_amd.capi._check
post = lambda: check(g.lib.hml_posterior(g.h, None, C.byref(loglik), C.byref(degenerate)))
counts = lambda: check(g.lib.hml_posterior_region_counts(g.h, N_REGIONS, start.ctypes.data, end.ctypes.data, H, hist.ctypes.data, ws.ctypes.data, av.ctypes.data, C.byref(bad)))
one = lambda: check(g.lib.hml_posterior_region_counts(g.h, 1, whole_start.ctypes.data, whole_end.ctypes.data, H, hist.ctypes.data, ws.ctypes.data, av.ctypes.data,
                                                      C.byref(bad)))
pairs = lambda: check(g.lib.hml_posterior_regions(g.h, N_REGIONS, start.ctypes.data, end.ctypes.data, whole.ctypes.data, ws.ctypes.data, eb.ctypes.data, share.ctypes.data,
                                                  None, C.byref(bad)))
sample = lambda: check(g.lib.hml_posterior_sample_regions(g.h, 0, DRAWS, 1, N_REGIONS, start.ctypes.data, end.ctypes.data, H, s_hist.ctypes.data, s_ws.ctypes.data,
                                                          s_sum.ctypes.data, s_sq.ctypes.data))
post()
t_post, t_counts = five(post), five(counts)
info = g.posterior_counts_info()
t_one = five(one)
info_one = g.posterior_counts_info()
t_pairs, t_sample = five(pairs), five(sample)
for label, t in (("hml_posterior", t_post), ("hml_posterior_region_counts", t_counts), ("... one whole-trace region", t_one), ("hml_posterior_regions", t_pairs),
                 ("hml_posterior_sample_regions", t_sample)):
    say("  %-30s %s ms   median %.2f" % (label, " ".join("%.2f" % v for v in t), statistics.median(t)))
base = statistics.median(t_post)
for label, t, i in (("20 000 regions", t_counts, info), ("one whole-trace region", t_one, info_one)):
    extra = statistics.median(t) - base
    say("  the terms and the walks of %s: %.2f ms beyond hml_posterior = %.2f of the smoothing pass; %d steps, the longest region %d: %.1f ns a step of the call, "
        "%.2f us a step of the longest chain" % (label, extra, extra / base, i["steps"], i["longest"], 1e6 * extra / max(i["steps"], 1), 1e3 * extra / max(i["longest"], 1)))
say("  %d pairs (b, i) without a usable u" % bad.value)
g.close()
write_out()

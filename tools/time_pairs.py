"""Cost of the pairwise read-outs of the smoothing (hml_posterior_breaks, hml_posterior_regions):
python tools/time_pairs.py [case ...]      (profiles/pairs_cost.txt)

Cases: the three of tools/time_posterior.py
       c3      config 3's chain, 10^8 positions, 5 states, dynamic blocks (about 1.8 10^5 blocks)
       dense   10^7 positions, every position a block (weights x 10^9)
       depth   simulated read depth of config 5's kind, 2.5 10^7 positions
Per case: the chain runs 30 sweeps, then hml_posterior without gamma - the yardstick: the smoothing pass both calls follow, in
the same build -, hml_posterior_breaks(0.5) and hml_posterior_regions with 20 000 random regions are each timed five times with
the host clock.  The new passes are what a call takes beyond hml_posterior.  Their traffic is counted as
  terms    the rows alpha and beta read once (16 B K bytes), a block's start and integral-array entries (4 + 16 D bytes), the
           2 K + 1 integer columns and p written (8 (2 K + 2) B)
  scans    the columns read twice and written once (24 (2 K + 1) B)
  breaks   p read twice (16 B);  regions: 2 (2 K + 1) words, 4 K doubles and two searches a region (not counted: 20 000 regions)
The lines are printed and written into profiles/pairs_cost.txt between the two marker lines "## tools/time_pairs.py: begin" and
"## tools/time_pairs.py: end" (the file is created with them if it is not there); what stands outside the markers - the summary,
a kernel trace, the benchmark's headlines - is written by hand and kept.  With `--kernels` nothing is timed by the host and
nothing is written: every call is made once, for a kernel trace of the caller's profiler."""
import ctypes as C, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import bench, hammlet_amd

CASES = {
    "c3": ("c3_1e8_k5_dynamic", None, False),
    "dense": ("c2_1e7_k5", None, True),
    "depth": ("c5_2.5e8_depth_k5", 25_000_000, False),
}
N_REGIONS = 20000
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "pairs_cost.txt")
BEGIN, END = "## tools/time_pairs.py: begin", "## tools/time_pairs.py: end"
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


args = [a for a in sys.argv[1:] if a != "--kernels"]
kernels_only = "--kernels" in sys.argv[1:]
for name in (args or list(CASES)):
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
    say("%s: T=%d K=%d blocks=%d regions=%d" % (name, T, K, B, N_REGIONS))
    rng = np.random.default_rng(1)
    start = rng.integers(0, T, N_REGIONS).astype(np.uint32)
    end = np.minimum(start.astype(np.int64) + rng.geometric(1e-5, N_REGIONS), T).astype(np.uint32)
    loglik, degenerate = C.c_double(), C.c_uint64()
    n, total, bad = C.c_uint64(), C.c_double(), C.c_uint64()
    whole, eb = np.empty(N_REGIONS), np.empty(N_REGIONS)
    ws, share = np.empty((N_REGIONS, K)), np.empty((N_REGIONS, K))
    check = hammlet_amd.capi._check
    post = lambda: check(g.lib.hml_posterior(g.h, None, C.byref(loglik), C.byref(degenerate)))
    # (pos == NULL: the count alone, so that the list's copy to the host is not what is timed; the full call is timed next to it)
    count = lambda: check(g.lib.hml_posterior_breaks(g.h, 0.5, C.byref(n), None, None, C.byref(total), C.byref(bad)))
    breaks = lambda: g.posterior_breaks(0.5)
    regions = lambda: check(g.lib.hml_posterior_regions(g.h, N_REGIONS, start.ctypes.data, end.ctypes.data, whole.ctypes.data, ws.ctypes.data, eb.ctypes.data,
                                                        share.ctypes.data, None, C.byref(bad)))
    if kernels_only:
        for call in (post, count, breaks, regions):
            call()
        g.close()
        continue
    post()
    t_post, t_count, t_breaks, t_regions = five(post), five(count), five(breaks), five(regions)
    for label, t in (("hml_posterior", t_post), ("hml_posterior_breaks, count", t_count), ("hml_posterior_breaks, list", t_breaks), ("hml_posterior_regions", t_regions)):
        say("  %-28s %s ms   median %.2f" % (label, " ".join("%.2f" % v for v in t), statistics.median(t)))
    base = statistics.median(t_post)
    terms = 16.0 * B * K + (4 + 16 * D) * B + 8.0 * (2 * K + 2) * B
    scans = 24.0 * (2 * K + 1) * B
    for label, t, traffic in (("breaks, count", t_count, terms + scans + 16.0 * B), ("regions", t_regions, terms + scans)):
        extra = statistics.median(t) - base
        say("  the new passes of %s: %.2f ms beyond hml_posterior = %.2f of the smoothing pass; %.1f MB counted, %.1f GB/s"
            % (label, extra, extra / base, traffic / 1e6, traffic / 1e9 / max(extra, 1e-6) * 1e3))
    say("  %d boundaries at or above 0.5, %.3f breakpoints expected, %d without a defined probability" % (n.value, total.value, bad.value))
    g.close()
    del x
if not kernels_only:
    write_out()

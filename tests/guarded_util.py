"""Shared by tests/test_gpu_guarded_memory.py and tests/test_guarded_memory_cpu.py: the cases of the full-capacity sweeps and a
walk of the configurations tests/fuzz_util.fuzz draws - on the CPU, nothing run - so that the seeds of the guarded fuzz slices
can be chosen, and shown to cover what the slices are there for, before anything runs on a GPU."""
import numpy as np

GUARD_BYTES = 4096

# every position a block (weights x 1e9): B = T = the capacity of the per-block arrays
LENGTHS = [1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097]
EVERY_K_AT = [1, 64, 65, 1025]           # lengths at which every number of states of a path runs


def spread(lengths, states, every_k_at=EVERY_K_AT):
    """(T, K) pairs: every K at the lengths of every_k_at, two K - another two from length to length - at the others"""
    out = []
    for i, T in enumerate(lengths):
        if T in every_k_at or len(states) <= 2:
            out += [(T, K) for K in states]
        else:
            out += [(T, states[(i + j) % len(states)]) for j in (0, len(states) // 2)]
    return out


def covers(pairs, lengths, states, every_k_at=EVERY_K_AT):
    """the rule the cases are drawn up by: every T with at least two K, every K at least at every_k_at"""
    for T in lengths:
        if len({K for t, K in pairs if t == T}) < min(2, len(states)):
            return False
    return all((T, K) in pairs for K in states for T in every_k_at if T in lengths)


DEFAULT_K = [2, 5, 7, 8, 16]
MID_K = [2, 5, 8, 16]
WEAK_LENGTHS = [T for T in LENGTHS if T >= 1023]
WEAK_K = [2, 5, 8, 16]
WIDE_K = [17, 20, 64]
COMPAT_K = [3, 20]
MANY_K = [3, 5]
GROWTH_LENGTHS = [64, 65, 1025]


# ------------------------------------------------------------------------------------------ the fuzz slices under the mode
# (count, seed, mode) per slice; the seeds were chosen with walk() below so that wanting() holds for the plain, compat and
# wide slices (tests/test_guarded_memory_cpu.py asserts it; a seed that misses is replaced, the thresholds stay)
FUZZ_SLICES = {
    "plain": (40, 20270101, {}),
    "max_blocks_64": (25, 20270201, {}),
    "many": (25, 20270301, dict(many=True)),
    "compat": (25, 20270401, dict(compat=True)),
    "wide": (30, 20270501, dict(wide=True)),
}
FUZZ_HOSTILE = [(30, 20270601, {}), (10, 20270602, dict(many=True)), (10, 20270603, dict(wide=True)), (10, 20270604, dict(compat=True))]
READOUT_SLICES = {
    "single_chain": (15, 20270701, {}),
    "batched_chains": (8, 20270702, dict(many=True)),
    "many_states": (8, 20270703, dict(wide=True)),
    "compat": (8, 20270704, dict(compat=True)),
    "hostile": (10, 20270705, dict(data="hostile")),
}


def walk(n_cfg, seed, compat=False, wide=False):
    """What tests/fuzz_util._fuzz draws for its first n_cfg configurations on Gaussian / read-depth data (data=None): the same
    draws from the same stream in the same order, nothing else.  Returns dicts T, K, D, dense, mult, scheme - the fields of the
    line _fuzz logs, which the GPU test compares them with."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_cfg):
        D = int(rng.choice([1, 1, 1, 2, 2, 3]))
        if D == 1:
            K = int(rng.integers(2, 17))
            if (compat and rng.random() < 0.3) or (wide and rng.random() < 0.5):
                K = int(rng.choice([17, 20, 31, 32, 33, 48, 64]))
        else:
            P = int(rng.choice(([2, 3, 4, 5, 7] if (compat or wide) else [2, 3, 4]) if D == 2 else ([2, 3] if (compat or wide) else [2])))
            K = P ** D
        T = int(rng.choice([17, 1000, 4097, 30000, 65535, 65537, 120000, 300000]))
        if K > 8 or D > 1:
            T = min(T, 120000)
        dense = bool(rng.random() < 0.3)
        mult = float(rng.choice([1.0, 1.0, 1.5, 1e9 if T <= 65537 else 1.0]))
        rng.random()                                         # self_trans
        for values in ([0.5, 0.1, 1.0], [0.5, 10.0], [0.5, 2.0], [0.2, 0.1], [0.9, 0.8]):     # t_off, t_diag, pi_alpha, e_var, e_p
            rng.choice(values)
        for values in ([8, 16, 32], [1, 1, 1, 0], [0, 32, 64, 96, 160, 256, 544, 1024], [1, 1, 1, 0], [1, 1, 0], [1, 1, 0]):
            rng.choice(values)                               # chunk of the dense filter, trellis switches, flag staging
        if rng.random() < 0.3:
            rng.choice([4, 8, 16])                           # warm-up
        for values in ([1, 1, 0], [4, 4, 1, 2, 8], [262144, 2000, 200]):
            rng.choice(values)                               # late rescale, forward chunk, mid geometry
        if compat or wide:
            rng.choice([None, None, 1, 7, 60, 500])
            rng.choice([None, None, -1, 1, 4])
            if wide:
                rng.choice([None, None, 1, 2, 4, 8, 64])
                rng.choice([None, None, None, 0])
            if K > 16:
                T = min(T, 65537)
        rng.integers(0, 1 << 30)                             # the chain's seed
        if rng.random() < 0.2 and D == 1:
            rng.integers(1, 100)                             # read depths
        else:
            for _d in range(D):
                rng.integers(1, 1000)
        scheme = []
        for _t in range(int(rng.integers(1, 5))):
            tok = rng.choice(["F", "F", "M", "S", "D", "P"])
            scheme.append((str(tok), int(rng.integers(1, 9)), int(rng.integers(0, 3))) if tok in ("F", "M") else str(tok))
        if not isinstance(scheme[-1], tuple):
            scheme.append(("F", int(rng.integers(1, 5)), 1))
        rng.choice([1, 1, 2, 0])                             # weight keys
        out.append(dict(T=T, K=K, D=D, dense=dense, mult=mult, scheme=scheme))
    return out


def line_of(c):
    """the part of _fuzz's log line that walk() foretells"""
    return "T=%d K=%d D=%d dense=%d mult=%g " % (c["T"], c["K"], c["D"], c["dense"], c["mult"]), "scheme=%s " % c["scheme"]


def wanting(lines):
    """What a slice must hold not to be hollow, counted on log lines (or on line_of's): at least 3 configurations where every
    position is a block, 3 on the weakly compressed geometry, 2 of several data dimensions, 2 schemes with a static block
    structure and 2 with a prior draw.  Returns the conditions that fail."""
    text = ["".join(l) if isinstance(l, tuple) else l for l in lines]
    schemes = [l.split("scheme=", 1)[1] for l in text if "scheme=" in l]
    dims = [int(l.split(" D=", 1)[1].split()[0]) for l in text if " D=" in l]
    have = {
        "mult=1e+09 >= 3": sum("mult=1e+09 " in l for l in text) >= 3,
        "dense=1 >= 3": sum("dense=1 " in l for l in text) >= 3,
        "D > 1 >= 2": sum(d > 1 for d in dims) >= 2,
        "S in scheme >= 2": sum("'S'" in s for s in schemes) >= 2,
        "P in scheme >= 2": sum("'P'" in s for s in schemes) >= 2,
    }
    return [k for k, ok in have.items() if not ok]


# ------------------------------------------------------------------------------------------ the recorders at full capacity
RECORDER_LENGTHS = [1, 2, 31, 32, 33, 65, 1025]
BAND_COLUMNS = 64                                   # hml_set_level_bands: data dimensions x (edges + 1) columns at most


def band_edges(D):
    """as many edges as the columns allow, 31 at most: 31 for one and two data dimensions (2 x 32 = all 64 columns), 20 for three"""
    return tuple(float(np.float32(v)) for v in np.linspace(-1.5, 1.5, min(31, BAND_COLUMNS // D - 1)))


BAND_EDGES = band_edges(1)


def record_all(T, n_chains=1, payload=True, D=3):
    """A record of tests/readout_fuzz_util.py made by hand: D data dimensions over two parameters (2 ** D states), every position a
    block, every recorder on from the start - as many band edges as band_edges(D) gives, the standard regions (the whole trace, its first and its last
    position among them) with two edges, the history at every sweep - through four tokens of nine sweeps, all recorded: 36 rows,
    which cross the history buffer's capacities of 16 and of 32.  (Those capacities are hml_history_ensure's, csrc/hml_readout.hip: at
    least 16 rows, doubled when a call's rows do not fit.  The 36 depends on them; test_history_buffer_grows_twice of
    tests/test_gpu_guarded_memory.py sees the two growths in the memory the library holds and fails if they stop happening.)  At the end the payloads go into a fresh context through buffers
    of exactly recording_payload_size bytes."""
    from tests import readout_fuzz_util as rf
    c = rf.configuration(20270801, T, many=n_chains > 1)
    c.update(D=D, P=2 if D > 1 else None, K=2 ** D if D > 1 else 5, T=T, data_kind="trace", levels=2, data_seed=5, n_chains=n_chains, attached=n_chains > 1, dense=False, mult=1e9,
             max_blocks=None, env={}, weight_keys=1, scheme=[("F", 9, 1), ("M", 9, 1), "S", ("F", 9, 1), "D", ("F", 9, 1)],
             on=[{r: True for r in rf.RECORDERS} for _ in range(n_chains)], band_edges=("values", band_edges(D)),
             region_edges=("values", (-0.5, 0.5)), every=1, flips={}, midrun={}, payload=payload, viterbi=(False, 1, 4), extra_chain=0)
    if D == 1:
        c.update(levels=5)
    return c


VIEW_CASES = [(1, 2), (33, 1), (33, 2), (1025, 1), (1025, 2)]      # (T, D); one observation of one dimension: the automatic prior refuses it


def view_record(T, D):
    """the record of the dense read-outs into caller-given memory: two dimensions - one chain of four states; one - two chains"""
    return record_all(T, n_chains=1 if D > 1 else 2, payload=False, D=D)      # (a batch is univariate)

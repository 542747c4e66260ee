"""Randomised differential run of the RECORDINGS: the read-outs beyond the reference - state marginals, emission levels,
breakpoints with consensus, level bands, regions, history, agreement, sparse payloads, Viterbi - with several recorders on at
once in one chain that goes through a random scheme of M / F / S / D / P tokens on every switchable sweep path, recorders
switched on and off between tokens, thinnings that do not divide a token's sweeps, read-outs taken in mid-run, graph replay,
tiny block capacities, batches of chains with different recorder sets.  Shared by tests/test_gpu_readout_fuzz.py (a bounded,
fixed-seed sample inside `-m gpu`), tests/test_readout_fuzz_cpu.py (the same sample on the checker alone: what it covers and that
it has something to find) and tools/fuzz_readouts.py (larger counts, by hand).

Two steps.  generate() is a pure function of (seed, index, mode): a configuration RECORD, a dict of plain values; configuration i
draws from default_rng([seed, i]) and its hostile input from a stream of its own, so one configuration can be replayed alone.
fuzz_readouts() consumes the records: the CPU checker goes through the scheme first (expectations()), one sweep per call
(tests/breaks_cases.checker_sweeps, tests/history_util.walk), then the GPU chain, and every comparison is made by the helper the
recorder's own test file uses - no expectation is restated here and no tolerance is new.

What a switch between tokens does (include/hml.h): a recorder that is off skips the recorded sweeps of the tokens it is off
for and keeps what it accumulated; the same edges / regions / `every` turn it on again.  So the expectation of a recorder is
the helper fed the checker's recorded sweeps of the tokens the recorder was on for."""
import math
import os
import tempfile
import time

import numpy as np

from tests import fuzz_util
from tests import hostile_inputs as hi
from tests import oracle_lib as ol

ENV_KEYS = tuple(fuzz_util.ENV_KEYS) + ("HML_USE_GRAPH",)
RECORDERS = ("marginals", "levels", "breaks", "bands", "regions", "history")
T_LIST = (33, 97, 1000, 4097, 8193, 30000, 65537)
READOUTS = ("levels_rle", "breaks_list", "breaks_consensus", "bands_rle", "bands_call", "regions", "history", "marginals_rle",
            "max_segmentation", "viterbi", "recording_export")
HOSTILE_TAG = 0x686f7374

# the bounded sample of tests/test_gpu_readout_fuzz.py and tests/test_readout_fuzz_cpu.py: test -> [(configurations, seed, mode)]
SAMPLES = {
    "single_chain": [(40, 20261201, {})],
    "batched_chains": [(15, 20261202, {"many": True})],
    "many_states": [(15, 20261203, {"wide": True})],
    "compat": [(15, 20261204, {"compat": True})],
    "hostile": [(20, 20261205, {"data": "hostile"}), (8, 20261206, {"many": True, "data": "hostile"})],
}


# ------------------------------------------------------------------------------------------------ 1. the generator (pure)
def generate(n_cfg, seed, many=False, compat=False, wide=False, data=None, only=None):
    """the configuration records 0 ... n_cfg - 1 of a seed and mode (only: that one alone)"""
    assert data in (None, "hostile"), data
    return [configuration(seed, i, many=many, compat=compat, wide=wide, data=data) for i in (range(n_cfg) if only is None else [only])]


def _pick(rng, values):
    """rng.choice over a list that may hold None; a plain Python value"""
    v = values[int(rng.integers(0, len(values)))]
    return v.item() if isinstance(v, np.generic) else v


def _scheme(rng):
    """2-5 tokens of F F M S D P, ending in a sweep token; 1-9 sweeps, thinning 0-4 (thinnings that do not divide stay in)"""
    scheme = []
    for _ in range(int(rng.integers(2, 6))):
        tok = _pick(rng, ["F", "F", "M", "S", "D", "P"])
        scheme.append((tok, int(rng.integers(1, 10)), int(rng.integers(0, 5))) if tok in ("F", "M") else tok)
    if not isinstance(scheme[-1], tuple):
        scheme[-1] = ("F", int(rng.integers(1, 10)), int(rng.integers(1, 5)))
    return scheme


def _edge_pick(rng, data_kind, levels, n_edges):
    """n_edges edges BETWEEN and INSIDE the trace's levels: ("values", ascending floats) for a Gaussian trace - the midpoints
    of neighbouring levels (a position's band differs between sweeps only near a change of level) and the levels themselves (the
    sampled mean of a state moves around its level: the band of a whole segment differs between sweeps); ("quantiles", ascending
    fractions of the data's distribution) for read depths and hostile inputs"""
    if n_edges == 0:
        return ("values", ())
    if data_kind == "trace":
        lv = sorted(ol.LEVELS[levels])
        cand = sorted(set(lv) | {(a + b) / 2.0 for a, b in zip(lv, lv[1:])})
        idx = np.sort(rng.choice(len(cand), size=min(n_edges, len(cand)), replace=False))
        return ("values", tuple(float(np.float32(cand[i] + rng.uniform(-0.003, 0.003))) for i in idx))
    return ("quantiles", tuple(sorted(float(q) for q in rng.uniform(0.05, 0.95, size=n_edges))))


def configuration(seed, index, many=False, compat=False, wide=False, data=None):
    rng = np.random.default_rng([seed, index])
    hostile = data == "hostile"
    c = dict(seed=seed, index=index, many=many, compat=compat, wide=wide, hostile=hostile)
    env = {}
    if many:
        D, P = 1, None
        K = _pick(rng, [2, 3, 4, 5, 5, 6, 8, 10, 13, 16])
    else:
        D = _pick(rng, [1, 1, 1, 2, 3])
        if D == 1:
            P, K = None, int(rng.integers(2, 17))
            if (compat and rng.random() < 0.3) or (wide and rng.random() < 0.5):
                K = _pick(rng, [17, 20, 33, 64])
        else:
            P = _pick(rng, [2, 3, 4])
            K = P ** D
    T = _pick(rng, list(T_LIST))
    if K > 8 or D > 1:
        T = min(T, 30000)
    levels = min(K if D == 1 else P, 5)
    kind = "depth" if (D == 1 and rng.random() < 0.2) else "trace"
    data_seed = int(rng.integers(1, 1000))
    if hostile:
        if D > 1:
            D, P, K = 1, None, min(K, 16)
        kind = "hostile"
        T = None                                                  # (drawn with the input, from the hostile stream: 2 ... 65537)
    c.update(D=D, P=P, K=K, T=T, data_kind=kind, levels=levels, data_seed=data_seed)
    if many:
        c["n_chains"] = int(rng.integers(2, 11))
        c["attached"] = bool(rng.random() < 0.75)
        mult = _pick(rng, [1.0, 1.0, 1.5])
        env.update({"HML_MANY_GROUPS": _pick(rng, [None, None, 1, 2, 3, 4]), "HML_FUSED_MANY_SLOTS": _pick(rng, [None, None, None, 2, 5]),
                    "HML_MAX_BLOCKS": _pick(rng, [None, None, 64]), "HML_FWD_CHUNK_MANY": _pick(rng, [None, None, 4, 16]),
                    "HML_DENSE_MIN_BLOCKS": _pick(rng, [1 << 22, 1 << 22, 1 << 22, 400]), "HML_LATE_RESCALE": _pick(rng, [1, 1, 0]),
                    "HML_FWD_WARMUP": _pick(rng, [None, None, 4, 8]), "HML_FM_SPLIT": _pick(rng, [None, None, 1, 0]),
                    "HML_FM_SPLIT_SUB": _pick(rng, [None, None, 2, 4])})
        c["dense"] = env["HML_DENSE_MIN_BLOCKS"] == 400
        c["max_blocks"] = None                                    # (the batch takes its capacity from the environment)
    else:
        c["n_chains"], c["attached"] = 1, False
        c["dense"] = bool(rng.random() < 0.3)
        mult = _pick(rng, [1.0, 1.0, 1.5, 1e9 if (T is not None and T <= 8193) else 1.0])
        env["HML_DENSE_MIN_BLOCKS"] = 500 if c["dense"] else 1 << 22
        env["HML_FWD_CHUNK_DENSE"] = _pick(rng, [8, 16, 32])
        env["HML_TRELLIS_FUSED"] = _pick(rng, [1, 1, 1, 0])
        env["HML_TRELLIS_L"] = _pick(rng, [0, 32, 64, 96, 160, 256, 544, 1024])
        env["HML_TRELLIS_ROWS"] = _pick(rng, [1, 1, 1, 0])
        env["HML_TRELLIS_CKPT"] = _pick(rng, [1, 1, 0])
        env["HML_TRELLIS_REFIT_ROUNDS"] = _pick(rng, [2, 2, 0, 1, 4, 3, 6])
        env["HML_STAGE_BITS"] = _pick(rng, [1, 1, 0])
        env["HML_FWD_WARMUP"] = _pick(rng, [4, 8, 16]) if rng.random() < 0.3 else None
        env["HML_LATE_RESCALE"] = _pick(rng, [1, 1, 0])
        env["HML_FWD_CHUNK"] = _pick(rng, [4, 4, 1, 2, 8])
        env["HML_MID_MIN_BLOCKS"] = _pick(rng, [262144, 2000, 200])
        if compat or wide:
            env["HML_COMPAT_CHUNKS"] = _pick(rng, [None, None, 1, 7, 60, 500])
            env["HML_COMPAT_WARMUP"] = _pick(rng, [None, None, -1, 1, 4])
            if wide:
                env["HML_WIDE"] = 1
                env["HML_WIDE_L"] = _pick(rng, [None, None, 1, 2, 4, 8, 64])
                env["HML_WIDE_LANES"] = _pick(rng, [None, None, None, 0])
        c["max_blocks"] = _pick(rng, [None, None, 64]) if D == 1 else None      # (option "max_blocks": univariate models)
    env["HML_USE_GRAPH"] = _pick(rng, [None, None, None, 1])
    c.update(env=env, mult=mult, weight_keys=_pick(rng, [1, 1, 2, 0]), chain_seed=int(rng.integers(0, 1 << 30)))
    scheme = c["scheme"] = _scheme(rng)
    # ---- the recorders: per chain which are on from the start; what they are given is the configuration's
    c["on"] = [{r: bool(rng.random() < 0.8) for r in RECORDERS} for _ in range(c["n_chains"])]
    if many:   # (launch masks that differ: a chain with no recorder and one with the history alone, where there is room)
        c["on"][int(rng.integers(0, c["n_chains"]))] = {r: False for r in RECORDERS}
        if c["n_chains"] > 2:
            c["on"][int(rng.integers(1, c["n_chains"]))] = {r: r == "history" for r in RECORDERS}
    c["band_edges"] = _edge_pick(rng, kind, levels, int(rng.integers(1, 5)))
    c["region_edges"] = _edge_pick(rng, kind, levels, int(rng.integers(0, 4)))
    c["region_seed"] = int(rng.integers(0, 1000))
    c["every"] = _pick(rng, [1, 2, 3])
    # ---- switches between tokens: sweep token index -> (chain, recorder, settle the chain first?) - half of the switches are
    # made behind sweeps that are still enqueued
    sweep_tokens = [k for k, tok in enumerate(scheme) if isinstance(tok, tuple)]
    c["flips"] = {}
    for k in sweep_tokens[1:]:
        if rng.random() < 0.25:
            c["flips"][k] = (int(rng.integers(0, c["n_chains"])), _pick(rng, list(RECORDERS)), bool(rng.random() < 0.5))
    # ---- read-outs in mid-run, behind ANY token (S, D and P included: rebuilt blocks, a pending prior draw): token index ->
    # (chain, read-out, payload kind).  The Viterbi decode needs the blocks of a sweep (include/hml.h): behind the first sweep token
    c["midrun"] = {}
    for k in range(len(scheme)):
        if rng.random() < 0.3:
            names = [n for n in READOUTS if n != "viterbi" or k >= sweep_tokens[0]]
            c["midrun"][k] = (int(rng.integers(0, c["n_chains"])), _pick(rng, names), int(rng.integers(0, 3)))
    # ---- the end of the configuration
    c["consensus"] = int(rng.integers(0, 3))
    c["dense_pick"] = int(rng.integers(0, 1 << 16))
    c["extra_chain"] = int(rng.integers(0, c["n_chains"]))
    c["payload"] = bool(rng.random() < 0.3)
    c["viterbi"] = (bool(rng.random() < 0.3), _pick(rng, [1, 64]), _pick(rng, [4, 64]))
    return c


def on_by_token(c):
    """per chain and recorder, per scheme token: is it on while that token runs"""
    state = [dict(on) for on in c["on"]]
    out = [{r: [] for r in RECORDERS} for _ in state]
    for k in range(len(c["scheme"])):
        if k in c["flips"]:
            chain, r, _ = c["flips"][k]
            state[chain][r] = not state[chain][r]
        for chain, st in enumerate(state):
            for r in RECORDERS:
                out[chain][r].append(st[r])
    return out


def describe(c, what=None, T=None):
    """the full description of a record; what, T: of its input (make_data) - a hostile input's family and length are drawn with it"""
    if what is None:
        try:
            what, _, T = make_data(c)
        except Exception:
            what, T = c["data_kind"], c["T"]
    env = {k[4:]: v for k, v in c["env"].items() if v is not None}
    on = " | ".join(",".join(r[:3] for r in RECORDERS if o[r]) or "-" for o in c["on"])
    return ("seed=%d index=%d %s%s T=%s K=%d D=%d chains=%d attached=%d mult=%g max_blocks=%s weight_keys=%d env=%s scheme=%s on=[%s] every=%d "
            "bands=%s region_edges=%s flips=%s midrun=%s payload=%d viterbi=%s") % (
        c["seed"], c["index"], "many " if c["many"] else "compat " if c["compat"] else "wide " if c["wide"] else "",
        ("hostile " if c["hostile"] else "") + what, T, c["K"], c["D"], c["n_chains"], c["attached"], c["mult"], c["max_blocks"], c["weight_keys"], env, c["scheme"], on, c["every"],
        c["band_edges"], c["region_edges"], c["flips"], c["midrun"], c["payload"], c["viterbi"])


# ------------------------------------------------------------------------------------------------ 2. the input and the checker
def make_data(c):
    """(description, float32 input, T) of a record: from the repository's generators alone"""
    if c["data_kind"] == "hostile":
        hrng = np.random.default_rng([c["seed"], c["index"], HOSTILE_TAG])
        T = int(hrng.choice([t for t in hi.FUZZ_T if 2 <= t <= (30000 if c["K"] > 8 else 65537)]))
        what, x = hi.fuzz_draw(hrng, T=T)
        return what, x, T
    T, D = c["T"], c["D"]
    if c["data_kind"] == "depth":
        return "depth", ol.synth_depth(T, seed=c["data_seed"] % 100 + 1), T
    x = np.stack([ol.trace(T, c["levels"], c["data_seed"] + d) for d in range(D)], axis=1).reshape(-1)
    return "trace", x, T


def edges_of(pick, x):
    kind, values = pick
    if kind == "values" or len(values) == 0:
        return tuple(values)
    e = np.unique(np.quantile(np.asarray(x, np.float64), values).astype(np.float32))
    e = e[np.isfinite(e)]
    return tuple(float(v) for v in e)


def case_of(c, x, T):
    """the record as a case of tests/breaks_cases.py / bands_cases.py"""
    return dict(T=T, K=c["K"], seed=c["chain_seed"], scheme=c["scheme"], trace=x, D=c["D"], P=c["P"], compat=c["compat"], env={},
                weight_mult=c["mult"], edges=edges_of(c["band_edges"], x))


class Refused(Exception):
    """the reference's own refusal of an input (autoprior): `both raise`"""


def expectations(c):
    """The checker through the record, one sweep per call, every chain run alone: dict(what, x, T, case, region_edges, regions,
    chains=[dict(sweeps=[per token: recorded sweeps], text=[per token: marginals text], blocks, states, theta, A, pi,
    rows, bounds, row_token)]).  Raises Refused with the checker's message where the reference refuses the input."""
    from tests import breaks_cases as bc
    from tests import history_util as hu
    from tests import regions_util as ru
    what, x, T = make_data(c)
    case = case_of(c, x, T)
    on = on_by_token(c)
    out = dict(what=what, x=x, T=T, case=case, region_edges=edges_of(c["region_edges"], x), chains=[], on=on)
    for chain in range(c["n_chains"]):
        try:
            o = bc.checker(case, chain=chain)
        except RuntimeError as err:
            raise Refused(str(err))
        e = dict(sweeps=[], text=[])
        try:
            for k, tok in enumerate(c["scheme"]):
                o.set_record(marginals=on[chain]["marginals"][k])
                e["sweeps"].append(bc.checker_sweeps(o, [tok], marginals=True))
                e["text"].append(o.text("marginals"))
            e["blocks"], e["states"], e["theta"] = o.blocks().copy(), o.states().copy(), o.theta().copy()
            e["A"], e["pi"] = o.transitions()
        finally:
            o.close()
        if any(on[chain]["history"]):
            o, prior = hu.checker(case, chain=chain)
            try:
                e["rows"], e["bounds"] = hu.walk(o, prior, c["scheme"], chain=chain, D=c["D"], P=c["P"])
            finally:
                o.close()
            e["row_token"] = np.concatenate([np.full(tok[1], k) for k, tok in enumerate(c["scheme"]) if isinstance(tok, tuple)])
        out["chains"].append(e)
    last = [s for per_token in out["chains"][0]["sweeps"] for s in per_token]
    last_sweep = last[-1] if last else (np.array([0, T]),)
    out["regions"] = ru.standard_regions(T, last_sweep, seed=c["region_seed"], n_random=40)
    return out


def sweeps_of(exp, chain, recorder, upto=None):
    """the checker's recorded sweeps of the tokens 0 ... upto that the recorder of the chain was on for"""
    per_token = exp["chains"][chain]["sweeps"]
    upto = len(per_token) - 1 if upto is None else upto
    return [s for k in range(upto + 1) if exp["on"][chain][recorder][k] for s in per_token[k]]


def history_rows(c, exp, chain, upto=None):
    """(rows, bounds) the history must hold after token `upto`: the sweeps whose number is a multiple of `every`, of the tokens
    the history was on for"""
    e = exp["chains"][chain]
    if "rows" not in e:
        return np.zeros((0, 11)), np.zeros((0, 11))
    upto = len(c["scheme"]) - 1 if upto is None else upto
    tok = e["row_token"]
    keep = (e["rows"][:, 0].astype(np.int64) % c["every"] == 0) & (tok <= upto) & np.array([exp["on"][chain]["history"][k] for k in tok], bool)
    return e["rows"][keep], e["bounds"][keep]


def asked(exp, chain, recorder, upto=None):
    """was the recorder ever on up to that token (its read-outs answer; otherwise they refuse)"""
    flags = exp["on"][chain][recorder]
    return any(flags[:(len(flags) if upto is None else upto + 1)])


# ------------------------------------------------------------------------------------------------ 3. the GPU run
_PROGRAM = {}


def viterbi_program():
    """the stand-alone restatement of the decode (tests/fixtures/viterbi_ref_main.cpp), built once per process"""
    if "exe" not in _PROGRAM:
        from tests import viterbi_util as vu
        _PROGRAM["dir"] = tempfile.TemporaryDirectory(prefix="viterbi_ref_")
        _PROGRAM["exe"] = vu.build_programs(_PROGRAM["dir"].name, sanitized=False)["plain"]
    return _PROGRAM["exe"]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _set_recorder(g, c, exp, recorder, flag):
    if recorder == "marginals":
        g.set_recording(marginals=flag)
    elif recorder == "levels":
        g.set_level_recording(flag)
    elif recorder == "breaks":
        g.set_break_recording(flag)
    elif recorder == "bands":
        g.set_level_bands(exp["case"]["edges"] if flag else ())
    elif recorder == "regions":
        if flag:
            g.set_regions(exp["regions"][0], exp["regions"][1], exp["region_edges"])
        else:
            g.set_regions((), ())
    else:
        g.set_history(flag, c["every"])


def _gpu_chains(hml, c, exp):
    """the GPU chains of a record, recorders as they are at the start; the reference's refusal must be the GPU's"""
    gs = []
    try:
        for chain in range(c["n_chains"]):
            g = hml.Chain(device=0, seed=c["chain_seed"], chain_id=chain)
            gs.append(g)
            if c["compat"]:
                g.set_option("compat", 1)
            g.set_option("weight_keys", c["weight_keys"])
            if c["max_blocks"]:
                g.set_option("max_blocks", c["max_blocks"])
            if c["attached"] and chain > 0:
                g.attach(gs[0])
            else:
                if c["D"] > 1:
                    g.set_dimensions(c["D"], c["P"])
                g.load(exp["x"])
                if c["mult"] != 1.0:
                    g.scale_weights(c["mult"])
            g.set_model(c["K"], g.autoprior(0.2, 0.9))
            for r in RECORDERS:
                if r == "marginals" or c["on"][chain][r]:
                    _set_recorder(g, c, exp, r, c["on"][chain][r])
            g._pending_prior = True
    except BaseException:
        for g in reversed(gs):   # (nothing created so far outlives a failure here)
            g.close()
        raise
    return gs


def _run_token(hml, c, gs, tok):
    for g in gs:
        if g._pending_prior:
            g.sample_prior()
            g._pending_prior = False
    if tok == "P":
        for g in gs:
            g._pending_prior = True
    elif tok == "S":
        for g in gs:
            g.set_static_blocks()
    elif tok == "D":
        for g in gs:
            g.set_dynamic(True)
    elif c["many"]:
        hml.iterate_many(gs, *tok)
    else:
        gs[0].iterate(*tok)


def check_recorder(hml, g, c, exp, chain, recorder, upto=None, what=""):
    """one recorder of one chain against the checker's sweeps so far, through the helper of the recorder's own tests"""
    from tests import bands_util as bdu
    from tests import breaks_cases as bc
    from tests import breaks_util as bu
    from tests import history_util as hu
    from tests import regions_util as ru
    from tests import test_gpu_bands as tb
    from tests import test_gpu_breaks as tk
    from tests import test_gpu_levels as tl
    case, T, D = exp["case"], exp["T"], c["D"]
    P = c["P"] if D > 1 else c["K"]
    if recorder == "marginals":
        assert hml.marginals_text(*g.marginals_rle()) == exp["chains"][chain]["text"][len(c["scheme"]) - 1 if upto is None else upto], (what, "marginals text")
        return
    if recorder == "history":
        rows, bounds = history_rows(c, exp, chain, upto)
        assert g.history_dropped() == 0, what
        hu.assert_rows(g.history(), rows, bounds, what=what + " history")
        return
    sweeps = sweeps_of(exp, chain, recorder, upto)
    if recorder == "levels":
        tl.assert_levels(g, sweeps, T, D=D, P=P, what=what + " levels")
    elif recorder == "breaks":
        C, N = bu.counts(sweeps, T)
        tk.assert_list(g, C, N, what + " breaks")
        tk.assert_consensus(g, C, N, [bc.CONSENSUS[c["consensus"]]], what + " consensus")
        if sweeps_of(exp, chain, "levels", upto):
            w, frac = bc.CONSENSUS[c["consensus"]]
            cuts = g.breaks_consensus(w, bu.min_count_of(frac, N))[0]
            tk.assert_on_segments(g, sweeps_of(exp, chain, "levels", upto), T, D, P, cuts.astype(np.int64), what + " levels on the consensus' segments")
    elif recorder == "bands":
        if not sweeps:   # asked, nothing recorded: one segment of zeros with N = 0 (include/hml.h)
            seg, cnt, n = g.bands_rle()
            assert n == 0 and list(seg) == [T] and not cnt.any(), what
            return
        length, want, N = tb.assert_bands(hml, g, sweeps, case, what=what + " bands")
        nb = len(case["edges"]) + 1
        for rank in (0, int(math.ceil(N / 2))):
            run_len, run_band = g.bands_call(rank)
            want_len, want_band = bdu.call(want, length, rank, D, nb)
            assert np.array_equal(run_len.astype(np.int64), want_len) and np.array_equal(run_band, want_band), (what, "bands_call", rank)
    elif recorder == "regions":
        want = ru.accumulate(sweeps, exp["regions"][0], exp["regions"][1], exp["region_edges"], D=D, P=(c["P"] if D > 1 else None))
        ru.assert_matches(g.regions(), want, what=what + " regions")


def _refused(hml, call, word, what):
    try:
        call()
    except hml.HmlError as err:
        assert err.code == 1 and word in str(err), (what, str(err))
        return
    raise AssertionError("%s: a read-out of a recorder that was never on did not refuse" % what)


NEVER = {"levels": "hml_set_level_recording", "breaks": "hml_set_break_recording", "bands": "hml_set_level_bands", "regions": "hml_set_regions"}


def midrun_readout(hml, g, c, exp, chain, name, kind, upto):
    """one read-out in the middle of the run, checked against the checker's sweeps so far; the run goes on behind it (and the
    checks at the end show that it changed nothing)"""
    from tests import test_gpu_recording_payload as tp
    from tests import viterbi_util as vu
    from hammlet_amd import chains as hc
    what = "mid-run after token %d, chain %d, %s" % (upto, chain, name)
    g.sync()
    recorder = {"levels_rle": "levels", "breaks_list": "breaks", "breaks_consensus": "breaks", "bands_rle": "bands", "bands_call": "bands",
                "regions": "regions", "history": "history", "marginals_rle": "marginals", "max_segmentation": "marginals"}.get(name)
    if name == "viterbi":
        from tests import test_gpu_viterbi as tv
        tv.check_decode(g, tv.reference(viterbi_program(), g), what)
    elif name == "recording_export":
        r = ("levels", "breaks", "bands")[kind]
        k = (hc.RECORDING_LEVELS, hc.RECORDING_BREAKS, hc.RECORDING_BANDS)[kind]
        if not asked(exp, chain, r, upto):
            _refused(hml, lambda: g.recording_payload_size(k), NEVER[r], what)
        else:
            p = hc.parse_recording_payload(tp.export(g, k))
            assert (p["kind"], p["T"], p["n_recorded"]) == (k, exp["T"], len(sweeps_of(exp, chain, r, upto))), what
            # its contents: the positions and raw cells of the chain's own run-length read-out (the layout test of
            # tests/test_gpu_recording_payload.py), which in turn is held against the checker's sweeps so far
            from tests import levels_util as lu
            pos = p["positions"].astype(np.int64)
            if p["n_recorded"] == 0:   # asked, nothing recorded yet: an empty payload
                assert p["M"] == 0, what
            elif r == "levels":
                seg, n, s1, s2 = g.levels_rle()
                assert np.array_equal(pos, tp.starts_of(seg)), what
                for d in range(c["D"]):
                    assert lu.exact_scan(p["cells"][2 * d]).tobytes() == s1[d].tobytes() and lu.exact_scan(p["cells"][2 * d + 1]).tobytes() == s2[d].tobytes(), (what, d)
            elif r == "breaks":
                bp, cnt, n = g.breaks_list()
                assert np.array_equal(p["positions"], bp) and np.array_equal(p["cells"][0], cnt), what
            else:
                seg, cnt, n = g.bands_rle()
                assert np.array_equal(pos, tp.starts_of(seg)) and np.array_equal(np.cumsum(p["cells"].astype(np.int64), axis=1).T, cnt.astype(np.int64)), what
            check_recorder(hml, g, c, exp, chain, r, upto=upto, what=what)
    elif name == "max_segmentation":
        run_len, run_state = g.max_segmentation()
        assert vu.tool_text(run_len, run_state) == ol.max_segmentation_text(exp["chains"][chain]["text"][upto]), what
    elif recorder in NEVER and not asked(exp, chain, recorder, upto):
        _refused(hml, {"levels": g.levels_rle, "breaks": g.breaks_list, "bands": g.bands_rle, "regions": g.regions}[recorder], NEVER[recorder], what)
    else:
        check_recorder(hml, g, c, exp, chain, recorder, upto=upto, what=what)


def check_chain(hml, g, c, exp, chain, what):
    """layers 1 and 2: the chain itself, then every recorder that was ever on"""
    e = exp["chains"][chain]
    g.sync()
    A, pi = g.transitions()
    same = (np.array_equal(e["blocks"], g.blocks()) and np.array_equal(e["states"], g.states()) and np.array_equal(_bits(e["theta"]), _bits(g.theta()))
            and np.array_equal(_bits(e["A"]), _bits(A)) and np.array_equal(_bits(e["pi"]), _bits(pi)))
    assert same, what + ": blocks, states, theta or A / pi differ from the checker's"
    check_recorder(hml, g, c, exp, chain, "marginals", what=what)
    # hml_recorded_sweeps is the marginals' own N: the sweeps recorded while the marginals flag was on (include/hml.h)
    assert g.recorded_sweeps() == len(sweeps_of(exp, chain, "marginals")), (what, "recorded_sweeps", g.recorded_sweeps(), len(sweeps_of(exp, chain, "marginals")))
    for r in RECORDERS[1:]:
        if asked(exp, chain, r):
            check_recorder(hml, g, c, exp, chain, r, what=what)
        elif r in NEVER:
            _refused(hml, {"levels": g.levels_rle, "breaks": g.breaks_list, "bands": g.bands_rle, "regions": g.regions}[r], NEVER[r], what + " " + r)
        else:
            assert g.history().shape == (0, 11), what


def check_dense(hml, g, c, exp, chain, what):
    """layer 3: the dense form of one recorder expanded from its run-length form (tests/test_gpu_readouts.py)"""
    import torch
    from tests import breaks_cases as bc
    from tests import breaks_util as bu
    from tests import test_gpu_breaks as tk
    from tests import test_gpu_readouts as tr
    T, D, K = exp["T"], c["D"], c["K"]
    have = ["marginals"] + [r for r in ("levels", "breaks", "bands") if asked(exp, chain, r)]
    r = have[c["dense_pick"] % len(have)]
    if r == "marginals":
        seg, cnt = g.marginals_rle()
        want = np.zeros((K + 1, T), np.int32)
        want[:cnt.shape[1]] = tr.expand(seg, cnt)
        want[K] = tr.start_indicator(seg, T) if cnt.shape[1] else 0
        out = torch.full((K + 1, T), -7, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()      # (the fill runs on torch's stream, the read-out on the chain's)
        g.marginals_dense_device(out.data_ptr())
        got = out.cpu().numpy()
        if cnt.shape[1] == 0:
            want[K] = got[K]                  # (nothing recorded: the counts are zero; the boundary row is not pinned by the header)
        assert np.array_equal(got, want), (what, "marginals dense")
    elif r == "levels":
        seg, n, s1, s2 = g.levels_rle()
        out = torch.full((2 * D, T), -7.0, dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()      # (the fill runs on torch's stream, the read-out on the chain's)
        g.levels_dense_device(out.data_ptr())
        got = out.cpu().numpy()
        if n == 0:   # nothing recorded: not-a-number everywhere (include/hml.h)
            assert np.all(np.isnan(got)), (what, "levels dense")
            return
        mean, sd = hml.levels_mean_sd(n, s1, s2)
        for d in range(D):
            assert np.array_equal(got[2 * d].view(np.uint32), np.repeat(mean[d], seg.astype(np.int64)).astype(np.float32).view(np.uint32)), (what, "levels dense", d)
            assert np.array_equal(got[2 * d + 1].view(np.uint32), np.repeat(sd[d], seg.astype(np.int64)).astype(np.float32).view(np.uint32)), (what, "levels dense", d)
    elif r == "breaks":
        C, N = bu.counts(sweeps_of(exp, chain, "breaks"), T)
        tk.assert_dense(g, C, N, [bc.DENSE_WINDOWS[c["dense_pick"] % 3]], what + " breaks dense")
    else:
        seg, cnt, n = g.bands_rle()
        out = torch.full((cnt.shape[1], T), -7, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()      # (the fill runs on torch's stream, the read-out on the chain's)
        g.bands_dense_device(out.data_ptr())
        assert np.array_equal(out.cpu().numpy(), tr.expand(seg, cnt).astype(np.int32)), (what, "bands dense")


def check_payloads(hml, g, c, exp, chain, what):
    """layer 4: each payload kind exported and merged into a context that loaded the same trace and recorded nothing: its
    read-outs are the source's, bit for bit"""
    from hammlet_amd import chains as hc
    from tests import test_gpu_recording_payload as tp
    fresh = hml.Chain(device=0, seed=c["chain_seed"], chain_id=chain + 100)
    try:
        if c["D"] > 1:
            fresh.set_dimensions(c["D"], c["P"])
        fresh.load(exp["x"])
        fresh.set_model(c["K"], fresh.autoprior(0.2, 0.9))
        for r, kind in (("levels", hc.RECORDING_LEVELS), ("breaks", hc.RECORDING_BREAKS), ("bands", hc.RECORDING_BANDS)):
            if not asked(exp, chain, r):
                continue
            tp.merge(fresh, kind, tp.export(g, kind))
            assert tp.readout(fresh, kind) == tp.readout(g, kind), (what, "payload of the " + r)
    finally:
        fresh.close()


def check_viterbi(hml, g, c, what):
    """layer 5: one decode against the stand-alone restatement, at a drawn launch geometry"""
    from tests import test_gpu_viterbi as tv
    g.set_option("viterbi_W", c["viterbi"][1])
    g.set_option("viterbi_L", c["viterbi"][2])
    tv.check(viterbi_program(), g, what=what + " viterbi")


def check_batch(hml, gs, c, exp, what):
    """the agreement of the chains that recorded levels, then the merges of chain 1 into chain 0 (or their documented refusals)"""
    from tests import regions_util as ru
    from tests import test_gpu_agreement as ta
    from tests import test_gpu_bands as tb
    from tests import test_gpu_breaks as tk
    from tests import test_gpu_levels as tl
    from tests import breaks_util as bu
    T, D = exp["T"], c["D"]
    n_lev = {ch: len(sweeps_of(exp, ch, "levels")) for ch in range(len(gs)) if asked(exp, ch, "levels")}
    for N in sorted(set(n_lev.values()), reverse=True):
        group = [ch for ch, n in n_lev.items() if n == N]
        if N >= 2 and len(group) >= 2:
            ta.assert_agreement(hml, [gs[ch] for ch in group], what + " agreement of chains %s" % group)
            break
    both = lambda r: sweeps_of(exp, 0, r) + sweeps_of(exp, 1, r)
    for r, merge, word in (("levels", gs[0].merge_levels, NEVER["levels"]), ("breaks", gs[0].breaks_merge, NEVER["breaks"]), ("bands", gs[0].merge_bands, NEVER["bands"])):
        if not asked(exp, 1, r):   # a source that never recorded: refused
            _refused(hml, lambda: merge(gs[1]), word, what + " merge of the " + r)
            continue
        merge(gs[1])
        if r == "levels":
            tl.assert_levels(gs[0], both(r), T, D=D, P=c["K"], what=what + " merged levels")
        elif r == "breaks":
            C, N = bu.counts(both(r), T)
            tk.assert_list(gs[0], C, N, what + " merged breaks")
        elif both(r):
            tb.assert_bands(hml, gs[0], both(r), exp["case"], what=what + " merged bands")
    if asked(exp, 0, "regions") and asked(exp, 1, "regions"):
        gs[0].regions_merge(gs[1])
        want = ru.accumulate(both("regions"), exp["regions"][0], exp["regions"][1], exp["region_edges"], D=D)
        ru.assert_matches(gs[0].regions(), want, what=what + " merged regions")      # (the bound holds for any order of the additions)
    else:
        _refused(hml, lambda: gs[0].regions_merge(gs[1]), "hml_set_regions", what + " merge of the regions")


def run_configuration(hml, c):
    """one record on the GPU against the checker: "ok", or "both raise: ..." where the reference refuses the input"""
    for k in ENV_KEYS:
        v = c["env"].get(k)
        fuzz_util._setenv(k, v)
    try:
        exp = expectations(c)
    except Refused as err:
        _, x, T = make_data(c)
        g = hml.Chain(device=0, seed=c["chain_seed"])
        try:
            g.load(x)
            if c["mult"] != 1.0:
                g.scale_weights(c["mult"])
            try:
                g.autoprior(0.2, 0.9)
            except hml.HmlError as gerr:
                assert str(err) in str(gerr), (str(err), str(gerr))
                return "both raise: %s" % err
            raise AssertionError("the checker raised %r, the GPU did not" % str(err))
        finally:
            g.close()
    gs = _gpu_chains(hml, c, exp)
    try:
        state = [dict(on) for on in c["on"]]
        for k, tok in enumerate(c["scheme"]):
            if k in c["flips"]:
                chain, r, settle = c["flips"][k]
                state[chain][r] = not state[chain][r]
                if settle:   # (otherwise the switch comes behind sweeps that are still enqueued: it governs the later ones only)
                    gs[chain].sync()
                _set_recorder(gs[chain], c, exp, r, state[chain][r])
            _run_token(hml, c, gs, tok)
            if k in c["midrun"]:
                chain, name, kind = c["midrun"][k]
                midrun_readout(hml, gs[chain], c, exp, chain, name, kind, k)
        for chain, g in enumerate(gs):
            check_chain(hml, g, c, exp, chain, "chain %d" % chain)
        x = c["extra_chain"]
        check_dense(hml, gs[x], c, exp, x, "chain %d" % x)
        if c["payload"]:
            check_payloads(hml, gs[x], c, exp, x, "chain %d" % x)
        if c["viterbi"][0]:
            check_viterbi(hml, gs[x], c, "chain %d" % x)
        if c["many"]:
            check_batch(hml, gs, c, exp, "batch")
    finally:
        for g in reversed(gs):
            g.close()
    return "ok"


def fuzz_readouts(hml, n_cfg, seed, many=False, compat=False, wide=False, data=None, log=None, only=None):
    """n_cfg random configurations of the recordings; returns the number that ran identical (all, or an AssertionError names the
    first that differs with its full description: replay it alone with tools/fuzz_readouts.py --seed S --only I).  The
    environment switches it sets are restored afterwards."""
    log = log or (lambda *a, **k: None)
    saved = {k: os.environ.get(k) for k in ENV_KEYS}
    t_start = time.time()
    try:
        for c in generate(n_cfg, seed, many=many, compat=compat, wide=wide, data=data, only=only):
            try:
                result = run_configuration(hml, c)
            except (AssertionError, hml.HmlError) as err:
                raise AssertionError("configuration %d DIFFERS: %s\n%s: %s" % (c["index"], describe(c), type(err).__name__, err)) from err
            log("%3d %s  %s  %.0f s" % (c["index"], result, describe(c), time.time() - t_start))
        return n_cfg
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v

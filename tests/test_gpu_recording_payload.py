"""Sparse payloads of the levels, breakpoints and bands on the GPU (hml_k_rec_payload.h behind hml_recording_payload_size /
hml_recording_export / hml_recording_merge_payload / hml_recording_merge_across).  The payloads are read and built by the numpy
mirror in hammlet_amd/chains.py; the expectations are the chains' own run-length read-outs, the existing same-device merges and
plain numpy - every comparison is bit for bit.  No test here asks the GPU for anything out of bounds: every refusal is a checked
argument error returned before a kernel writes."""
import numpy as np
import pytest
import torch

from hammlet_amd import chains as hc
from tests import levels_util as lu
from tests import oracle_lib as ol

pytestmark = pytest.mark.gpu

L, B, LB = hc.RECORDING_LEVELS, hc.RECORDING_BREAKS, hc.RECORDING_BANDS
KINDS = (L, B, LB)
EDGES = np.array([-0.5, 0.5], np.float32)
GUARD = 64
SCHEME = [("F", 12, 1)]


def gpu_chain(hml, K, seed, x=None, chain=0, D=1, P=None, attach=None, record=True, device=0, edges=EDGES):
    g = hml.Chain(device=device, seed=seed, chain_id=chain)
    if attach is not None:
        g.attach(attach)
    else:
        if D > 1:
            g.set_dimensions(D, P)
        g.load(x)
    g.set_model(K, g.autoprior(0.2, 0.9))
    if record:
        g.set_level_recording(True)
        g.set_break_recording(True)
        g.set_level_bands(edges)
    g.sample_prior()
    return g


def run(g, scheme=SCHEME):
    for tok in scheme:
        g.iterate(*tok)
    g.sync()
    return g


def export(g, kind, device="cuda:0"):
    """the chain's payload as a uint8 array, through a device buffer with guard bytes behind it"""
    n = g.recording_payload_size(kind)
    buf = torch.full((n + GUARD,), 0xA5, dtype=torch.uint8, device=device)
    torch.cuda.synchronize()
    assert g.recording_export(kind, buf.data_ptr(), n) == n
    host = buf.cpu().numpy()
    assert np.all(host[n:] == 0xA5)
    return host[:n].copy()


def merge(g, kind, payload, n_bytes=None, device="cuda:0"):
    t = torch.from_numpy(np.ascontiguousarray(payload, np.uint8)).to(device)
    torch.cuda.synchronize()
    g.recording_merge_payload(kind, t.data_ptr(), t.numel() if n_bytes is None else n_bytes)


def readout(g, kind):
    """every run-length read-out of a kind and its N, as bytes"""
    if kind == L:
        seg, n, s1, s2 = g.levels_rle()
        return (n, seg.tobytes(), s1.tobytes(), s2.tobytes())
    if kind == B:
        pos, cnt, n = g.breaks_list()
        return (n, pos.tobytes(), cnt.tobytes()) + tuple(a.tobytes() for a in g.breaks_consensus(16, 1))
    seg, cnt, n = g.bands_rle()
    return (n, seg.tobytes(), cnt.tobytes()) + tuple(a.tobytes() for a in g.bands_call(0))


def starts_of(seg):
    seg = seg.astype(np.int64)
    return np.cumsum(seg) - seg


# ---------------------------------------------------------------------------------------- 1. layout
LAYOUT = {
    "T30000_K4": dict(T=30000, K=4),
    "T97_K4": dict(T=97, K=4),            # not a multiple of 32
    "T4097_K4": dict(T=4097, K=4),        # crosses one span of 4096 positions
    "T4097_D2": dict(T=4097, K=4, D=2, P=2),
    "T30000_K20": dict(T=30000, K=20),    # the many-states path
}


def layout_chain(hml, c):
    T, K, D = c["T"], c["K"], c.get("D", 1)
    if D > 1:
        x = np.stack([ol.trace(T, c["P"], 9 + d) for d in range(D)], axis=1).reshape(-1)
    else:
        x = ol.trace(T, 4, 7)
    return run(gpu_chain(hml, K, 21, x, D=D, P=c.get("P")))


@pytest.mark.parametrize("name", list(LAYOUT))
def test_layout_of_an_exported_payload(hml, name):
    c = LAYOUT[name]
    T, D = c["T"], c.get("D", 1)
    g = layout_chain(hml, c)
    for kind in KINDS:
        p = hc.parse_recording_payload(export(g, kind))
        rows = {L: 2 * D, B: 1, LB: D * (len(EDGES) + 1)}[kind]
        assert (p["kind"], p["T"], p["rows"], p["cell_bytes"]) == (kind, T, rows, (8, 4, 4)[kind]), (name, kind)
        assert p["n_recorded"] == 12 and p["M"] == len(p["positions"])
        if kind == LB:
            assert p["n_edges"] == len(EDGES) and p["edges"].tobytes() == EDGES.tobytes() and not p["edge_slots"][len(EDGES):].view(np.uint32).any()
        else:
            assert p["n_edges"] == 0 and not p["edge_slots"].view(np.uint32).any()
        pos = p["positions"].astype(np.int64)
        assert np.all(np.diff(pos) > 0) and (p["M"] == 0 or pos[-1] < T)
        if kind == L:
            seg, n, s1, s2 = g.levels_rle()
            assert n == 12 and np.array_equal(pos, starts_of(seg)) and pos[0] == 0, name
            for d in range(D):   # the read-out's fixed tree over the raw cells gives the read-out's sums, bit for bit
                assert lu.exact_scan(p["cells"][2 * d]).tobytes() == s1[d].tobytes(), (name, d)
                assert lu.exact_scan(p["cells"][2 * d + 1]).tobytes() == s2[d].tobytes(), (name, d)
            assert not np.any(np.signbit(p["cells"]) & (p["cells"] == 0.0))     # a cell is never -0.0
        elif kind == B:
            bp, cnt, n = g.breaks_list()
            assert n == 12 and np.array_equal(p["positions"], bp) and np.array_equal(p["cells"][0], cnt), name
            assert p["M"] == 0 or pos[0] > 0
        else:
            seg, cnt, n = g.bands_rle()
            assert n == 12 and np.array_equal(pos, starts_of(seg)) and pos[0] == 0, name
            assert np.array_equal(np.cumsum(p["cells"].astype(np.int64), axis=1).T, cnt.astype(np.int64)), name
        print("%s kind %d: M = %d, %d bytes" % (name, kind, p["M"], hc.recording_payload_size(p["M"], rows, p["cell_bytes"])))
    if name == "T30000_K4":
        assert hc.parse_recording_payload(export(g, L))["M"] > 1


def test_a_recorder_that_was_asked_but_recorded_nothing_exports_an_empty_payload(hml):
    g = gpu_chain(hml, 4, 3, ol.trace(4097, 4, 7))
    for kind in KINDS:
        p = hc.parse_recording_payload(export(g, kind))
        assert (p["M"], p["n_recorded"], p["T"]) == (0, 0, 4097) and g.recording_payload_size(kind) == 192
    never = gpu_chain(hml, 4, 3, attach=g, record=False)
    for kind, word in ((L, "hml_set_level_recording"), (B, "hml_set_break_recording"), (LB, "hml_set_level_bands")):
        with pytest.raises(hml.HmlError) as e:
            never.recording_payload_size(kind)
        assert e.value.code == 1 and word in str(e.value)


# ---------------------------------------------------------------------------------------- 2. hand-made payloads
def hand_made(kind, T, M, seed):
    """a payload of M positions with the extreme ones (0 for levels and bands, T - 1) among them, and its parts"""
    rng = np.random.default_rng(seed)
    lo = 1 if kind == B else 0
    inner = np.arange(lo + 1, T - 1)
    ends = [lo, T - 1][:M] if kind != B else [T - 1][:M]
    pos = np.sort(np.concatenate([ends, rng.choice(inner, size=M - len(ends), replace=False)])).astype(np.uint32)
    rows = {L: 2, B: 1, LB: len(EDGES) + 1}[kind]
    if kind == L:
        cells = rng.standard_normal((rows, M))
    elif kind == B:
        cells = rng.integers(1, 9, (rows, M)).astype(np.uint32)
    else:
        cells = rng.integers(-5, 6, (rows, M)).astype(np.int32)
    n = 7 + M
    return hc.recording_payload(kind, T, pos, cells, n, EDGES if kind == LB else None), pos, cells, n


@pytest.mark.parametrize("T", [97, 4097])
def test_hand_made_payloads_into_fresh_contexts(hml, T):
    base = gpu_chain(hml, 4, 5, ol.trace(T, 4, 7), record=False)
    for M in (0, 1, 2, 63, 64, 65, 257):
        if M > T - 1:
            continue
        g = gpu_chain(hml, 4, 5, attach=base, chain=1, record=False)
        for kind in KINDS:
            buf, pos, cells, n = hand_made(kind, T, M, 1000 * kind + M + T)
            assert buf.size == 192 + 8 * ((M + 1) // 2) + cells.shape[0] * M * cells.dtype.itemsize
            merge(g, kind, buf)
            pos = pos.astype(np.int64)
            with_zero = pos if (M and pos[0] == 0) else np.concatenate([[0], pos])
            dense = np.zeros((cells.shape[0], T), cells.dtype)
            dense[:, pos] = cells
            if kind == L:
                seg, got_n, s1, s2 = g.levels_rle()
                assert got_n == n and np.array_equal(starts_of(seg), with_zero) and seg.sum() == T, (T, M)
                assert s1[0].tobytes() == lu.exact_scan(dense[0, with_zero]).tobytes(), (T, M)
                assert s2[0].tobytes() == lu.exact_scan(dense[1, with_zero]).tobytes(), (T, M)
            elif kind == B:
                bp, cnt, got_n = g.breaks_list()
                assert got_n == n and np.array_equal(bp, pos) and np.array_equal(cnt, cells[0]), (T, M)
            else:
                seg, cnt, got_n = g.bands_rle()
                assert got_n == n and np.array_equal(starts_of(seg), with_zero) and seg.sum() == T, (T, M)
                assert np.array_equal(cnt.astype(np.int64), np.cumsum(dense.astype(np.int64), axis=1)[:, with_zero].T), (T, M)
                assert np.array_equal(g.level_bands(), EDGES)      # a destination without edges takes the payload's
            # ... and what was merged comes out again as it went in (levels and bands: with the position 0 that is always listed)
            back = hc.parse_recording_payload(export(g, kind))
            want_pos = pos if kind == B else with_zero
            assert back["n_recorded"] == n and np.array_equal(back["positions"], want_pos), (T, M, kind)
            assert back["cells"].tobytes() == np.ascontiguousarray(dense[:, want_pos]).tobytes(), (T, M, kind)


# ---------------------------------------------------------------------------------------- 3. equivalence with the same-device merges
def trio(hml, x, ids=(0, 1, 2)):
    first = run(gpu_chain(hml, 4, 13, x, chain=ids[0]))
    return [first] + [run(gpu_chain(hml, 4, 13, attach=first, chain=ch)) for ch in ids[1:]]


def test_payload_merge_equals_the_existing_merge(hml):
    x = ol.trace(30000, 4, 7)
    a, b, c = trio(hml, x)
    a1, b1, c1 = trio(hml, x)
    a2, b2, c2 = trio(hml, x)
    for kind in KINDS:
        assert readout(a, kind) == readout(a1, kind) == readout(a2, kind) and readout(b, kind) != readout(a, kind)
    a.merge_levels(b); a.merge_levels(c)
    a.breaks_merge(b); a.breaks_merge(c)
    a.merge_bands(b); a.merge_bands(c)
    for kind in KINDS:
        before = [readout(b1, kind), readout(c1, kind)]
        for src in (b1, c1):
            merge(a1, kind, export(src, kind))
        for src in (b2, c2):
            a2.recording_merge_across(src, kind)
        want = readout(a, kind)
        assert want[0] == 36, kind                                # N of the three chains
        assert readout(a1, kind) == want, kind
        assert readout(a2, kind) == want, kind
        assert [readout(b1, kind), readout(c1, kind)] == before   # the sources are only read
        # ... down to the raw cells: the merged recorders export the same payload
        assert export(a, kind).tobytes() == export(a1, kind).tobytes() == export(a2, kind).tobytes(), kind
    # the merged chain records on
    a1.iterate("F", 2, 1)
    a1.sync()
    assert a1.levels_rle()[1] == 38 and a1.breaks_list()[2] == 38 and a1.bands_rle()[2] == 38


def test_the_numpy_mirror_merges_like_the_device(hml):
    x = ol.trace(4097, 4, 7)
    a, b, c = trio(hml, x)
    fresh = gpu_chain(hml, 4, 13, attach=a, chain=9, record=False)
    for kind in KINDS:
        parts = [export(g, kind) for g in (a, b, c)]
        for p in parts:
            merge(fresh, kind, p)
        assert export(fresh, kind).tobytes() == hc.merge_recording_payloads(parts).tobytes(), kind


def test_pooled_recording_of_a_single_process(hml):
    """without a process group hammlet_amd.chains.pooled_recording gathers the chain's own payload and merges nothing"""
    a = run(gpu_chain(hml, 4, 13, ol.trace(4097, 4, 7)))
    for kind in KINDS:
        before = readout(a, kind)
        parts = hc.pooled_recording(a, kind)
        assert len(parts) == 1 and parts[0].cpu().numpy().tobytes() == export(a, kind).tobytes()
        assert readout(a, kind) == before


# ---------------------------------------------------------------------------------------- 4. shadow contexts
def test_a_shadow_context_reads_out_like_the_source(hml):
    x = ol.trace(30000, 4, 7)
    a, b, _ = trio(hml, x)
    shadow = gpu_chain(hml, 4, 13, attach=a, chain=1, record=False)       # observations, model, no sweep
    merge(shadow, L, export(b, L))
    assert readout(shadow, L) == readout(b, L) and readout(b, L)[0] == 12
    one, two = hml.levels_agreement_rle([a, b]), hml.levels_agreement_rle([a, shadow])
    assert one[1] == two[1] == 12 and len(one[0]) > 1
    for u, v in zip(one, two):
        assert np.asarray(u).tobytes() == np.asarray(v).tobytes()
    for u, v in zip(hml.levels_agreement_summary([a, b], 1.1), hml.levels_agreement_summary([a, shadow], 1.1)):
        assert u.tobytes() == v.tobytes()


# ---------------------------------------------------------------------------------------- 5. refusals
def test_refusals_leave_the_destination_untouched(hml):
    T = 4097
    x = ol.trace(T, 4, 7)
    dst, src, _ = trio(hml, x)
    before = [readout(dst, kind) for kind in KINDS]
    raw_before = [export(dst, kind).tobytes() for kind in KINDS]
    good = {kind: export(src, kind) for kind in KINDS}
    assert all(hc.parse_recording_payload(good[kind])["M"] >= 3 for kind in KINDS)
    messages = []

    def refused(kind, payload, n_bytes=None):
        with pytest.raises(hml.HmlError) as e:
            merge(dst, kind, payload, n_bytes)
        assert e.value.code == 1, str(e.value)
        messages.append(str(e.value))
        assert [readout(dst, k) for k in KINDS] == before, str(e.value)
        assert [export(dst, k).tobytes() for k in KINDS] == raw_before, str(e.value)

    def patched(kind, word, value):
        p = good[kind].copy()
        p[:64].view("<u8")[word] = value
        return p

    def with_positions(kind, change):
        p = good[kind].copy()
        M = hc.parse_recording_payload(p)["M"]
        change(p[192:192 + 4 * M].view("<u4"))
        return p

    bad = good[L].copy()
    bad[0] ^= 0x01
    refused(L, bad)                                                    # bad magic
    refused(B, good[L])                                                # wrong kind
    refused(L, patched(L, 2, T + 1))                                   # wrong T
    refused(L, patched(L, 3, 4))                                       # wrong rows
    refused(L, good[L], n_bytes=good[L].size - 8)                      # n_bytes short by 8

    def swap(pos):
        pos[1], pos[2] = pos[2], pos[1]
    refused(L, with_positions(L, swap))                                # positions out of order

    def last_is_T(pos):
        pos[-1] = T
    refused(LB, with_positions(LB, last_is_T))                         # a position equal to T

    def first_is_zero(pos):
        pos[0] = 0
    refused(B, with_positions(B, first_is_zero))                       # a breaks payload holding position 0
    edge = good[LB].copy()
    edge[64:68].view("<u4")[0] ^= 1
    refused(LB, edge)                                                  # bands edges differing in one bit
    # export with a capacity one below the size: nothing is written, also not behind the buffer
    n = src.recording_payload_size(L)
    buf = torch.full((n + GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    with pytest.raises(hml.HmlError) as e:
        src.recording_export(L, buf.data_ptr(), n - 1)
    assert e.value.code == 1
    messages.append(str(e.value))
    assert np.all(buf.cpu().numpy() == 0xA5)
    print("\n".join(messages))
    assert len(messages) == 10 and len(set(messages)) == 10, messages
    # ... and the destination still takes the good payloads
    for kind in KINDS:
        merge(dst, kind, good[kind])
        assert readout(dst, kind)[0] == 24


# ---------------------------------------------------------------------------------------- 6. two GPUs
def test_merge_across_two_gpus(hml):
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    x = ol.trace(30000, 4, 7)
    a, b = trio(hml, x, ids=(0, 1))
    a_far = run(gpu_chain(hml, 4, 13, x, chain=0))
    b_far = run(gpu_chain(hml, 4, 13, x, chain=1, device=1))
    a.merge_levels(b); a.breaks_merge(b); a.merge_bands(b)
    for kind in KINDS:
        assert readout(b_far, kind) == readout(b, kind)
        a_far.recording_merge_across(b_far, kind)
        assert readout(a_far, kind) == readout(a, kind) and readout(a, kind)[0] == 24, kind
        assert export(a_far, kind).tobytes() == export(a, kind).tobytes(), kind

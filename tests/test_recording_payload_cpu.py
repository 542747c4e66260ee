"""The sparse payload of a recording (include/hml.h, hml_recording_export) on the CPU: the numpy mirror in hammlet_amd/chains.py
- size formula, build -> parse round trip for the three kinds, the merge of several payloads against a dense numpy sum - and the
all-gather of payloads of unequal length over a world-size-2 gloo group, started the way tests/test_pooling_gloo.py starts its ranks."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from hammlet_amd import chains

L, B, LB = chains.RECORDING_LEVELS, chains.RECORDING_BREAKS, chains.RECORDING_BANDS
EDGES = np.array([-0.5, 0.25, 1.5], np.float32)


def random_payload(kind, T, M, seed, D=1, edges=EDGES, first=None):
    """a payload of M random positions (levels and bands: position 0 among them) with random cells; returns it with its parts"""
    rng = np.random.default_rng(seed)
    lo = 1 if kind == B else 0
    pos = np.sort(rng.choice(np.arange(lo, T), size=M, replace=False)).astype(np.uint32)
    if first is not None and M:
        pos[0] = first
    rows = {L: 2 * D, B: 1, LB: D * (len(edges) + 1)}[kind]
    if kind == L:
        cells = rng.standard_normal((rows, M))
    elif kind == B:
        cells = rng.integers(1, 50, (rows, M)).astype(np.uint32)
    else:
        cells = rng.integers(-20, 20, (rows, M)).astype(np.int32)
    n = int(rng.integers(1, 100))
    return chains.recording_payload(kind, T, pos, cells, n, edges if kind == LB else None), pos, cells, n


@pytest.mark.parametrize("M", [0, 1, 2, 63, 64, 65, 257])
def test_size_formula_for_odd_and_even_M(M):
    for kind, rows, cell in ((L, 2, 8), (L, 4, 8), (B, 1, 4), (LB, 4, 4), (LB, 8, 4)):
        want = 192 + 8 * ((M + 1) // 2) + rows * M * cell
        assert chains.recording_payload_size(M, rows, cell) == want
        D = rows // 2 if kind == L else rows // 4 if kind == LB else 1
        buf, pos, cells, n = random_payload(kind, 4097, M, 3 + M, D=D, first=None if kind == B else 0)
        assert buf.dtype == np.uint8 and buf.size == want
        if M % 2 == 1:                               # the padding behind an odd number of positions is zero
            assert not buf[192 + 4 * M: 192 + 4 * (M + 1)].any()


@pytest.mark.parametrize("kind", [L, B, LB])
def test_build_parse_round_trip(kind):
    for T, M, D in ((97, 5, 1), (97, 96, 2), (4097, 65, 1), (4097, 0, 2)):
        buf, pos, cells, n = random_payload(kind, T, M, 11 * M + T + kind, D=D)
        p = chains.parse_recording_payload(buf)
        assert (p["kind"], p["T"], p["M"], p["n_recorded"]) == (kind, T, M, n)
        assert p["rows"] == cells.shape[0] and p["cell_bytes"] == chains.RECORDING_CELL[kind].itemsize
        assert np.array_equal(p["positions"], pos) and p["cells"].dtype == chains.RECORDING_CELL[kind]
        assert p["cells"].tobytes() == np.ascontiguousarray(cells).tobytes()
        if kind == LB:
            assert p["n_edges"] == 3 and p["edges"].tobytes() == EDGES.tobytes() and not p["edge_slots"][3:].any()
        else:
            assert p["n_edges"] == 0 and not p["edge_slots"].view(np.uint32).any()
        # the header as the 8 little-endian words of include/hml.h
        head = np.frombuffer(buf[:64].tobytes(), "<u8")
        assert head[0] == 0x00314345524C4D48 and bytes(buf[:8]) == b"HMLREC1\0"
        assert list(head[1:]) == [kind, T, cells.shape[0], M, n, p["cell_bytes"], p["n_edges"]]
        # bytes, a torch tensor and the array parse alike
        for other in (buf.tobytes(), torch.from_numpy(buf)):
            q = chains.parse_recording_payload(other)
            assert np.array_equal(q["positions"], pos) and q["cells"].tobytes() == p["cells"].tobytes()
    with pytest.raises(ValueError):
        chains.parse_recording_payload(buf[:-8])
    bad = buf.copy()
    bad[0] ^= 1
    with pytest.raises(ValueError):
        chains.parse_recording_payload(bad)


@pytest.mark.parametrize("kind", [L, B, LB])
@pytest.mark.parametrize("overlap", ["overlapping", "disjoint"])
def test_merge_against_a_dense_sum(kind, overlap):
    T, D = 4097, 2
    rng = np.random.default_rng(5 + kind)
    parts, dense, total = [], None, 0
    for j in range(3):
        if overlap == "disjoint":
            pool = np.arange(1, T)[j::3]
        else:
            pool = np.arange(1, 400)
        pos = np.sort(rng.choice(pool, size=130 + j, replace=False)).astype(np.uint32)
        buf, _, cells, n = random_payload(kind, T, len(pos), 100 * kind + j, D=D)
        buf = chains.recording_payload(kind, T, pos, cells, n, EDGES if kind == LB else None)
        parts.append(buf)
        if dense is None:
            dense = np.zeros((cells.shape[0], T), cells.dtype)
        dense[:, pos] = dense[:, pos] + cells          # (list order: the doubles of the levels do not commute bit for bit)
        total += n
    m = chains.parse_recording_payload(chains.merge_recording_payloads(parts))
    union = np.unique(np.concatenate([chains.parse_recording_payload(p)["positions"] for p in parts]))
    assert np.array_equal(m["positions"], union) and m["n_recorded"] == total and m["T"] == T and m["kind"] == kind
    assert m["cells"].tobytes() == np.ascontiguousarray(dense[:, union]).tobytes()
    untouched = np.ones(T, bool)
    untouched[union] = False
    assert not dense[:, untouched].any()
    if overlap == "disjoint":
        assert len(union) == sum(chains.parse_recording_payload(p)["M"] for p in parts)
    else:
        assert len(union) < sum(chains.parse_recording_payload(p)["M"] for p in parts)
    # one payload merges to itself; payloads over other positions are refused
    assert chains.merge_recording_payloads([parts[0]]).tobytes() == parts[0].tobytes()
    other, _, _, _ = random_payload(kind, T + 1, 4, 1, D=D)
    with pytest.raises(ValueError):
        chains.merge_recording_payloads([parts[0], other])


def rank_payload(rank):
    """rank 0: 5 level positions; rank 1: 64 - payloads of unequal length"""
    return random_payload(L, 4097, 5 if rank == 0 else 64, 40 + rank, first=0)[0]


def worker(rank, world, port, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    got = chains.gather_recording_payloads(torch.from_numpy(rank_payload(rank)))
    np.savez(out % rank, **{"p%d" % r: g.numpy() for r, g in enumerate(got)})
    dist.barrier()
    dist.destroy_process_group()


def test_gather_of_unequal_payloads_world2(tmp_path):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    out = str(tmp_path / "gathered%d.npz")
    mp.spawn(worker, args=(2, port, out), nprocs=2, join=True)
    want = [rank_payload(0), rank_payload(1)]
    assert want[0].size != want[1].size
    for rank in range(2):
        got = np.load(out % rank)
        assert sorted(got.files) == ["p0", "p1"]
        for r in range(2):
            assert got["p%d" % r].dtype == np.uint8 and got["p%d" % r].tobytes() == want[r].tobytes(), (rank, r)
            assert chains.parse_recording_payload(got["p%d" % r])["M"] == (5, 64)[r]
    # without a process group: the payload itself
    t = torch.from_numpy(want[0])
    assert chains.gather_recording_payloads(t)[0] is t

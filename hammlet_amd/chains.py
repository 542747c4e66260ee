"""Chain-parallel execution: independent Gibbs chains, one per GPU (one process per GPU), and the single collective of
the design - a sum all-reduce that pools the chains' state marginals at the end.

The product path is the C ABI: `hml_pool_create` / `hml_pool_marginals` (RCCL over xGMI inside libhammlet_hip.so,
hammlet_amd.Pool here) or `hml_allreduce_marginals` for one process that drives several GPUs.  This module holds the
launcher glue around it - how the ranks of a torch.distributed job obtain the RCCL id - and a tensor-level mirror of the
payload algebra (`payload_from_dense`, `pool_payload`, `payload_to_rle`) that works on any backend, which is how the
world-size-2 gloo test on CPU covers the N > 1 semantics (relabel, sum, cut at the union of the boundaries).

The label-free recordings - emission levels, breakpoint counts, level bands - cross GPUs as SPARSE PAYLOADS (include/hml.h,
hml_recording_export / hml_recording_merge_payload): `recording_payload`, `parse_recording_payload` and
`merge_recording_payloads` are the numpy mirror of that layout and of the merge, `gather_recording_payloads` the all-gather
of payloads of unequal length on any backend, `pooled_recording` the product path of one process per GPU.

The reference has nothing distributed (one process, one thread, src/main.cpp:108).  Pooling needs (1) a common
labelling of the states - every chain relabels its states by ascending emission mean, the idea of the reference's
bin/sortStates:1-6 - and (2) one all-reduce over the int32 payload [K+1][T+1] (+ K+1 words): K relabelled difference
arrays of the recorded marginals, one row that is non-zero at segment boundaries, the number of recorded sweeps and
which states were ever recorded (hammlet_amd/csrc/hml_k_pool.h).
"""
import numpy as np


def relabel_permutation(means):
    """perm[new] = old such that the states are ordered by ascending mean (ties keep their order); `means` may be
    [K] or, for "-s C P D" states, [K][D] tuples of mapped parameter means compared in dimension order"""
    means = np.asarray(means, np.float64)
    if means.ndim == 1:
        return np.argsort(means, kind="stable").astype(np.int32)
    return np.lexsort(tuple(means[:, d] for d in range(means.shape[1] - 1, -1, -1))).astype(np.int32)


def payload_from_dense(dense, boundary, perm, n_recorded):
    """The int32 payload of one chain from dense per-position counts [K][T], a 0/1 boundary row [T], the relabelling
    and the number of recorded sweeps - what hml_pool_export builds on the device from the difference arrays."""
    dense = np.asarray(dense, np.int64)
    K, T = dense.shape
    d = dense[np.asarray(perm)]
    diff = np.zeros((K + 1, T + 1), np.int64)
    diff[:K, 0] = d[:, 0]
    diff[:K, 1:T] = d[:, 1:] - d[:, :-1]
    diff[K, :T] = np.asarray(boundary) != 0
    diff[K, 0] = 1
    used = (d != 0).any(axis=1).astype(np.int64)
    return np.concatenate([diff.ravel(), [n_recorded], used]).astype(np.int32)


def pool_payload(payload, group=None):
    """Sum all-reduce of a payload tensor over the process group (in place).  Works on any backend: "nccl" (= RCCL on
    ROCm) for device tensors, "gloo" for the CPU tests.  (The product path does this inside the library.)"""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
        dist.all_reduce(payload, op=dist.ReduceOp.SUM, group=group)
    return payload


def list_from_dense(dense, boundary, perm, n_recorded):
    """The boundary list of one chain (hml_k_pool_list_pack): header [M, recorded sweeps, used[0..K-1]], then for every
    marginal segment [position, deltas of the relabelled states] - the non-zero columns of payload_from_dense's arrays."""
    dense = np.asarray(dense, np.int64)
    K, T = dense.shape
    pay = payload_from_dense(dense, boundary, perm, n_recorded).astype(np.int64)
    body = pay[: (K + 1) * (T + 1)].reshape(K + 1, T + 1)
    pos = np.flatnonzero(body[K, :T])
    entries = np.concatenate([pos[:, None], body[:K, pos].T], axis=1)
    return np.concatenate([[len(pos), n_recorded], pay[(K + 1) * (T + 1) + 1:], entries.ravel()]).astype(np.int32)


def pool_lists(lst, K, group=None):
    """All-gather of the ranks' boundary lists in equally sized slots (the library: ncclAllGather; here any backend).
    Returns the list of all ranks' lists."""
    import torch
    import torch.distributed as dist
    t = torch.as_tensor(lst, dtype=torch.int32)
    if not (dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1):
        return [t]
    world = dist.get_world_size(group)
    m = torch.tensor([int(t[0])], dtype=torch.int64)
    dist.all_reduce(m, op=dist.ReduceOp.MAX, group=group)
    slot = 2 + K + int(m.item()) * (K + 1)
    mine = torch.zeros(slot, dtype=torch.int32)
    mine[: t.numel()] = t
    out = [torch.zeros(slot, dtype=torch.int32) for _ in range(world)]
    dist.all_gather(out, mine, group=group)
    return out


def payload_from_lists(lists, K, T):
    """The pooled dense payload from all ranks' boundary lists: every entry added into zeroed arrays
    (hml_k_pool_list_install) - equal to the sum of the ranks' dense payloads."""
    import torch
    body = torch.zeros((K + 1, T + 1), dtype=torch.int64)
    rec, used = 0, torch.zeros(K, dtype=torch.int64)
    for l in lists:
        l = torch.as_tensor(l).to(torch.int64)
        M = int(l[0])
        rec += int(l[1])
        used += l[2:2 + K]
        e = l[2 + K: 2 + K + M * (K + 1)].view(M, K + 1)
        body[:K].index_put_((torch.arange(K)[None, :].expand(M, K), e[:, :1].expand(M, K)), e[:, 1:], accumulate=True)
        body[K, e[:, 0]] += 1
    body[K, 0] = max(int(body[K, 0]), 1)
    return torch.cat([body.flatten(), torch.tensor([rec]), used]).to(torch.int32)


def payload_to_rle(payload, K, T):
    """Run-length form of a pooled payload: prefix sums of the difference rows, cut wherever the boundary row is
    non-zero; columns up to the highest state any chain recorded (reference src/StateMarginals.hpp:300-303).
    Returns (segment lengths [M], counts [M][columns], recorded sweeps)."""
    import torch
    body = payload[: (K + 1) * (T + 1)].view(K + 1, T + 1)
    tail = payload[(K + 1) * (T + 1):]
    flags = body[K, :T] != 0
    flags[0] = True
    starts = torch.nonzero(flags, as_tuple=False).flatten()
    ends = torch.cat([starts[1:], torch.tensor([T], device=payload.device, dtype=starts.dtype)])
    dense = torch.cumsum(body[:K, :T].to(torch.int64), dim=1)
    used = torch.nonzero(tail[1:1 + K] != 0, as_tuple=False).flatten()
    cols = int(used.max().item()) + 1 if used.numel() else 0
    counts = dense[:cols, starts].t().contiguous()
    return (ends - starts), counts, int(tail[0].item())


def max_segmentation(seg, cnt):
    """Maximum-posterior-margin segmentation of (pooled) run-length marginals - the reference's post-processing tool
    (reference src/tools/maxSegmentation.cpp:53-82) on tensors: arg-max state per segment (first maximum; state 0 for
    an all-zero row), adjacent segments of equal state merged.  Returns (run lengths, run states) on seg's device."""
    import torch
    if cnt.shape[1] == 0:
        state = torch.zeros(seg.shape[0], dtype=torch.int64, device=seg.device)
    else:
        best = cnt.max(dim=1, keepdim=True).values
        # first column that reaches the maximum; a row without a positive count gives column 0 like the tool's `>`
        first = (cnt == best).to(torch.int8).argmax(dim=1)
        state = torch.where(best.flatten() > 0, first, torch.zeros_like(first))
    keep = torch.ones_like(state, dtype=torch.bool)
    keep[1:] = state[1:] != state[:-1]
    starts = torch.nonzero(keep, as_tuple=False).flatten()
    csum = torch.cat([torch.zeros(1, dtype=seg.dtype, device=seg.device), torch.cumsum(seg, 0)])
    ends = torch.cat([starts[1:], torch.tensor([seg.shape[0]], device=seg.device, dtype=starts.dtype)])
    return csum[ends] - csum[starts], state[starts]


def make_pool(device, group=None, always_broadcast=False):
    """The RCCL communicator of this rank inside a torch.distributed job (one process per GPU): rank 0 creates the id,
    the job's own backend broadcasts its 128 bytes, every rank joins (ncclCommInitRank).  Without an initialised
    process group: a one-rank communicator.  always_broadcast: take the broadcast path in a one-rank group as well
    (rehearsal of the multi-rank path on one GPU)."""
    import torch.distributed as dist
    from .capi import Pool
    if dist.is_available() and dist.is_initialized() and (dist.get_world_size(group) > 1 or always_broadcast):
        rank, world = dist.get_rank(group), dist.get_world_size(group)
        box = [Pool.unique_id() if rank == 0 else None]
        dist.broadcast_object_list(box, src=0, group=group)
        return Pool(device, rank, world, box[0])
    return Pool(device, 0, 1, Pool.unique_id())


def pooled_marginals(chain, pool):
    """Pools the recorded marginals of all chains of the communicator (hml_pool_marginals) and returns the pooled
    run-length marginals (segment lengths, counts) together with the permutation this chain applied."""
    perm = pool.marginals(chain)
    seg, cnt = chain.marginals_rle()
    return seg, cnt, perm


# ---- sparse payloads of the levels, breakpoints and bands (include/hml.h; csrc/hml_k_rec_payload.h) ----
RECORDING_MAGIC = 0x00314345524C4D48           # the bytes "HMLREC1\0"
RECORDING_LEVELS, RECORDING_BREAKS, RECORDING_BANDS = 0, 1, 2
RECORDING_CELL = {RECORDING_LEVELS: np.dtype("<f8"), RECORDING_BREAKS: np.dtype("<u4"), RECORDING_BANDS: np.dtype("<i4")}
_REC_FIXED = 192                               # 8 uint64 of header, 32 floats of edges


def recording_payload_size(M, rows, cell_bytes):
    """192 + 8 ceil(M / 2) + rows M (bytes per cell)"""
    return _REC_FIXED + 8 * ((int(M) + 1) // 2) + int(rows) * int(M) * int(cell_bytes)


def recording_payload(kind, T, positions, cells, n_recorded, edges=None):
    """The payload hml_recording_export writes, as a uint8 array: `positions` [M] ascending, `cells` [rows][M] the raw cells of
    the recorder there (float64 for levels, uint32 for breaks, int32 for bands), `edges` the bands' edges.  Nothing is checked
    here - the library checks what it is given - so that faulty payloads can be built as well."""
    cell = RECORDING_CELL[kind]
    pos = np.ascontiguousarray(positions, "<u4").reshape(-1)
    M = pos.size
    cells = np.ascontiguousarray(cells, cell)
    cells = cells.reshape(-1, M) if M else cells.reshape(cells.shape[0] if cells.ndim == 2 else 0, 0)
    rows = cells.shape[0]
    e = np.zeros(32, "<f4")
    n_edges = 0
    if edges is not None:
        edges = np.ascontiguousarray(edges, "<f4").reshape(-1)
        n_edges = edges.size
        e[:n_edges] = edges
    head = np.array([RECORDING_MAGIC, kind, T, rows, M, n_recorded, cell.itemsize, n_edges], "<u8")
    padded = np.zeros(2 * ((M + 1) // 2), "<u4")
    padded[:M] = pos
    out = np.concatenate([head.view(np.uint8), e.view(np.uint8), padded.view(np.uint8), cells.reshape(-1).view(np.uint8)])
    assert out.size == recording_payload_size(M, rows, cell.itemsize)
    return out


def parse_recording_payload(buf):
    """dict(kind, T, rows, M, n_recorded, cell_bytes, n_edges, edges[n_edges], edge_slots[32], positions[M], cells[rows][M]) of a
    payload given as bytes, a uint8 array or a uint8 tensor on the host; raises ValueError on a buffer that is not one"""
    buf = np.frombuffer(bytes(buf), np.uint8) if isinstance(buf, (bytes, bytearray, memoryview)) else np.ascontiguousarray(np.asarray(buf), np.uint8).reshape(-1)
    if buf.size < _REC_FIXED:
        raise ValueError("shorter than the header of a recording's payload")
    head = buf[:64].view("<u8")
    if int(head[0]) != RECORDING_MAGIC:
        raise ValueError("not a recording's payload: wrong magic number")
    kind, T, rows, M, N, cell_bytes, n_edges = (int(v) for v in head[1:8])
    if kind not in RECORDING_CELL or RECORDING_CELL[kind].itemsize != cell_bytes:
        raise ValueError("unknown kind or cell size")
    if buf.size != recording_payload_size(M, rows, cell_bytes):
        raise ValueError("the size is not the one the header implies")
    slots = buf[64:_REC_FIXED].view("<f4").copy()
    off = _REC_FIXED
    pos = buf[off:off + 4 * M].view("<u4").copy()
    off += 8 * ((M + 1) // 2)
    cells = buf[off:].view(RECORDING_CELL[kind]).reshape(rows, M).copy()
    return {"kind": kind, "T": T, "rows": rows, "M": M, "n_recorded": N, "cell_bytes": cell_bytes, "n_edges": n_edges,
            "edges": slots[:n_edges].copy(), "edge_slots": slots, "positions": pos, "cells": cells}


def merge_recording_payloads(payloads):
    """What a recorder holds after the payloads were merged into a fresh one, in list order, as a payload again: the union of
    the positions, the cells added in list order starting from zero (the order matters for the levels' doubles), the counts of
    recorded sweeps summed.  The payloads must agree in kind, T, rows and edges."""
    parts = [p if isinstance(p, dict) else parse_recording_payload(p) for p in payloads]
    a = parts[0]
    for p in parts[1:]:
        if (p["kind"], p["T"], p["rows"]) != (a["kind"], a["T"], a["rows"]) or p["edge_slots"].tobytes() != a["edge_slots"].tobytes():
            raise ValueError("payloads of different kinds, positions, rows or edges")
    union = np.unique(np.concatenate([p["positions"] for p in parts])) if parts else np.zeros(0, np.uint32)
    cells = np.zeros((a["rows"], union.size), RECORDING_CELL[a["kind"]])
    for p in parts:
        idx = np.searchsorted(union, p["positions"])
        cells[:, idx] = cells[:, idx] + p["cells"]
    return recording_payload(a["kind"], a["T"], union, cells, sum(p["n_recorded"] for p in parts), a["edges"] if a["n_edges"] else None)


def gather_recording_payloads(tensor, group=None):
    """All-gather of the ranks' payloads (1-D uint8 tensors of unequal length): first the sizes, then the payloads padded with
    zeros to the longest; returns every rank's payload, unpadded, in rank order - on every rank.  Any backend: "gloo" with
    host tensors, "nccl" (= RCCL on ROCm) with tensors of the rank's GPU.  Without a process group: [tensor]."""
    import torch
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1):
        return [tensor]
    world = dist.get_world_size(group)
    size = torch.tensor([tensor.numel()], dtype=torch.int64, device=tensor.device)
    sizes = [torch.zeros(1, dtype=torch.int64, device=tensor.device) for _ in range(world)]
    dist.all_gather(sizes, size, group=group)
    sizes = [int(s.item()) for s in sizes]
    slot = max(sizes)
    mine = torch.zeros(slot, dtype=torch.uint8, device=tensor.device)
    mine[: tensor.numel()] = tensor
    out = [torch.zeros(slot, dtype=torch.uint8, device=tensor.device) for _ in range(world)]
    dist.all_gather(out, mine, group=group)
    return [o[:n] for o, n in zip(out, sizes)]


def pooled_recording(chain, kind, group=None, root=0):
    """One process per GPU: every rank exports its chain's recording of `kind`, the payloads are gathered over the group
    (device tensors: the group's backend must move them, i.e. "nccl"), and rank `root` merges the other ranks' payloads into
    its chain in ascending rank order (hml_recording_merge_payload); the other ranks' chains are left as they were.  Returns the
    gathered payloads in rank order."""
    import torch
    import torch.distributed as dist
    dev = torch.device("cuda", chain.device)
    n = chain.recording_payload_size(kind)
    buf = torch.zeros(n, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)              # (the chain writes on its own stream)
    chain.recording_export(kind, buf.data_ptr(), n)
    parts = gather_recording_payloads(buf, group)
    torch.cuda.synchronize(dev)
    rank = dist.get_rank(group) if dist.is_available() and dist.is_initialized() else 0
    if rank == root:
        for r, part in enumerate(parts):
            if r != rank:
                part = part.contiguous()
                chain.recording_merge_payload(kind, part.data_ptr(), part.numel())
    return parts


def gathered_history(chain, group=None):
    """One process per GPU: every rank's history rows (Chain.history(), float64 [n_r, 11]) gathered on the CPU, in rank order, on
    every rank - a list of arrays.  The group's backend moves host tensors ("gloo"), or device tensors of the rank's GPU
    ("nccl").  Without a process group: [chain.history()].  hammlet_amd.history_stats takes one column of the list's arrays,
    cut to their common length: np.stack([h[-n:, col] for h in rows])."""
    import torch
    import torch.distributed as dist
    rows = np.ascontiguousarray(chain.history())
    if not (dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1):
        return [rows]
    raw = torch.from_numpy(rows.view(np.uint8).reshape(-1).copy())
    if dist.get_backend(group) == "nccl":
        raw = raw.to(torch.device("cuda", chain.device))
    parts = gather_recording_payloads(raw, group)
    return [p.cpu().numpy().view(np.float64).reshape(-1, rows.shape[1]) for p in parts]

#!/usr/bin/env python3
"""Neighbour sampling (gcn_amd.sample_neighbors / sample_blocks, gcn_amd/csrc/sample.hip) on the headline graph
(Reddit-shaped, graphgen.make_graph("reddit")): 1024 shuffled seeds with fanouts [25, 10] — a training batch — and 65536
seeds with fanout [10].  Per case: the selection kernels alone (the C entry point on a prepared out_rowptr, CUDA events),
sample_neighbors with its Python layer and host synchronisation, sample_blocks as a whole (wall clock: it synchronises),
and the plan build of a block's CsrAdjacency (wall clock) — the share a throw-away block pays before its first SpMM.
The yardstick is the same contract in torch ops on the same GPU: a Philox key per entry of the seeds' rows, a stable sort by
(row, key), the first f of every row, a sort back into entry order; its result must equal the kernel's, integer for integer.
Prints one JSON line and writes it to the profiles directory as sampling_bench_reddit.json (--out FILE: elsewhere).

    python tools/sampling_bench.py [--steps 20] [--warmup 5] [--scale 1.0] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import gcn_amd                  # noqa: E402
from gcn_amd import _lib, graphgen    # noqa: E402
from gcn_amd.spmm import _ptr, _stream_ptr    # noqa: E402

MASK = 0xFFFFFFFF


def events_ms(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) / steps, 4)


def wall_ms(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return round((time.perf_counter() - t0) * 1e3 / steps, 4)


def _mulhilo(a, b):
    """the 64-bit product of the 32-bit constant a and the 32-bit values b (int64 tensor) as (hi, lo) words"""
    bl, bh = b & 0xFFFF, b >> 16
    pl, ph = a * bl, a * bh                               # each below 2^48
    mid = ph + (pl >> 16)
    return mid >> 16, ((mid & 0xFFFF) << 16) | (pl & 0xFFFF)


def torch_keys(e, seed, offset):
    """key(e) of the contract in torch ops (int64 tensors holding 32-bit words)"""
    j = e >> 2
    c0, c1 = j & MASK, j >> 32
    c2 = torch.full_like(j, offset & MASK)
    c3 = torch.full_like(j, offset >> 32)
    k0, k1 = seed & MASK, seed >> 32
    for _ in range(10):
        hi0, lo0 = _mulhilo(0xD2511F53, c0)
        hi1, lo1 = _mulhilo(0xCD9E8D57, c2)
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + 0x9E3779B9) & MASK, (k1 + 0xBB67AE85) & MASK
    w = e & 3
    return torch.where(w == 0, c0, torch.where(w == 1, c1, torch.where(w == 2, c2, c3)))


def torch_sample(adj, seeds, fanout, seed, offset):
    """the contract in torch ops → (rowptr, col, eid) like gcn_amd.sample_neighbors"""
    s = seeds.long()
    rp = adj.rowptr.long()
    b, d = rp[s], rp[s + 1] - rp[s]
    ns, total = int(s.numel()), int(d.sum())
    starts = torch.cumsum(d, 0) - d
    rows = torch.repeat_interleave(torch.arange(ns, device=s.device), d, output_size=total)
    e = b[rows] + torch.arange(total, device=s.device) - starts[rows]
    order = torch.sort((rows << 32) | torch_keys(e, seed, offset), stable=True).indices   # by (row, key, entry)
    rank = torch.arange(total, device=s.device) - starts[rows]      # (rows is sorted: position i belongs to rows[i])
    taken = e[order][rank < fanout]
    taken_rows = rows[rank < fanout]                      # (the sort kept the rows in place)
    eid = torch.sort((taken_rows << 32) | taken).values & MASK
    out_rowptr = torch.zeros(ns + 1, dtype=torch.int32, device=s.device)
    out_rowptr[1:] = torch.cumsum(d.clamp(max=fanout), 0)
    return out_rowptr, adj.col[eid], eid.to(torch.int32)


def torch_blocks(adj, seeds, fanouts, seed, offset, vmap):
    """sample_blocks with torch_sample in the place of the kernel (the same relabelling ops)"""
    dst = seeds.long()
    for hop, f in enumerate(fanouts):
        _, col, _ = torch_sample(adj, dst, f, seed, offset + hop)
        vmap[dst] = torch.arange(dst.numel(), dtype=torch.int32, device=dst.device)
        c = col.long()
        new = torch.unique(c[vmap[c] < 0])
        src = torch.cat([dst, new])
        vmap[src] = -1
        dst = src
    return dst


def measure(adj, seeds, fanouts, steps, warmup):
    dev = seeds.device
    f, seed, offset = fanouts[0], 1, 0
    rowptr, col, eid = gcn_amd.sample_neighbors(adj, seeds, f, seed, offset)
    s32 = seeds.to(torch.int32)
    ws = torch.empty(_lib.SAMPLE_WS_BYTES, dtype=torch.uint8, device=dev)
    lib = _lib.load()

    def kernel():
        lib.gcn_sample_neighbors_csr(_ptr(adj.rowptr), _ptr(adj.col), adj.m, adj.nnz, _ptr(s32), s32.numel(), f, seed, offset,
                                     _ptr(rowptr), _ptr(col), _ptr(eid), _ptr(ws), ws.numel(), _stream_ptr(dev))

    lens = (adj.rowptr[seeds.long() + 1] - adj.rowptr[seeds.long()]).long()
    row = {"seeds": int(seeds.numel()), "fanouts": list(fanouts), "entries_in_seed_rows": int(lens.sum()),
           "longest_seed_row": int(lens.max()), "rows_over_long_limit": int((lens > _lib.SAMPLE_LONG_ROW).sum()),
           "sampled_entries": int(col.numel()),
           "kernel_ms": events_ms(kernel, steps, warmup),
           "sample_neighbors_ms": wall_ms(lambda: gcn_amd.sample_neighbors(adj, seeds, f, seed, offset), steps, warmup),
           "sample_blocks_ms": wall_ms(lambda: gcn_amd.sample_blocks(adj, seeds, fanouts, seed, offset), steps, warmup)}
    ref = torch_sample(adj, seeds, f, seed, offset)
    row["equals_torch"] = all(bool(torch.equal(a, b)) for a, b in zip((rowptr, col, eid), ref))
    few = max(2, min(steps, 5))
    row["torch_sample_ms"] = wall_ms(lambda: torch_sample(adj, seeds, f, seed, offset), few, 1)
    vmap = torch.full((adj.n,), -1, dtype=torch.int32, device=dev)
    row["torch_blocks_ms"] = wall_ms(lambda: torch_blocks(adj, seeds, fanouts, seed, offset, vmap), few, 1)
    row["torch_sample_over_kernel"] = round(row["torch_sample_ms"] / row["kernel_ms"], 1)
    row["torch_sample_over_sample_neighbors"] = round(row["torch_sample_ms"] / row["sample_neighbors_ms"], 2)
    row["torch_blocks_over_sample_blocks"] = round(row["torch_blocks_ms"] / row["sample_blocks_ms"], 2)
    blocks, input_ids = gcn_amd.sample_blocks(adj, seeds, fanouts, seed, offset)
    blk = blocks[0]                                       # the outermost block: the largest

    def plan():
        gcn_amd.CsrAdjacency(blk.adj.rowptr, blk.adj.col, blk.adj.val, (blk.adj.m, blk.adj.n), symmetric=False).plan

    row["block_shape"] = [blk.adj.m, blk.adj.n, blk.adj.nnz]
    row["input_vertices"] = int(input_ids.numel())
    row["block_plan_build_ms"] = wall_ms(plan, few, 1)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rowptr, col, val, n = graphgen.make_graph("reddit", device=dev, seed=1, scale=args.scale)
    adj = gcn_amd.CsrAdjacency(rowptr, col, val, (n, n), symmetric=True)
    gen = torch.Generator(device="cpu")
    gen.manual_seed(0)
    perm = torch.randperm(n, generator=gen).to(dev)
    res = {"graph": "reddit", "scale": args.scale, "n": n, "nnz": adj.nnz, "steps": args.steps, "warmup": args.warmup,
           "long_row_limit": _lib.SAMPLE_LONG_ROW,
           "what": "ms per call; kernel_ms: CUDA events around the C entry point alone; the others wall clock, host "
                   "synchronisations included; torch_*: the same contract in torch ops",
           "cases": []}
    ok = True
    for count, fanouts in ((1024, [25, 10]), (65536, [10])):
        row = measure(adj, perm[:min(count, n)], fanouts, args.steps, args.warmup)
        ok = ok and row["equals_torch"]
        res["cases"].append(row)
        print(f"# {row}", file=sys.stderr, flush=True)
    res["error_check"] = "pass" if ok else "FAIL"
    line = json.dumps(res)
    print(line)
    out = args.out or os.path.join(ROOT, "profiles", "sampling_bench_reddit.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Induced-subgraph extraction (gcn_amd.induced_subgraph, gcn_amd/csrc/subgraph.hip) on the headline graph (Reddit-shaped,
graphgen.make_graph("reddit")) for three vertex sets: 2 000 and 20 000 random vertices — GraphSAINT-sized batches, almost
every entry of the touched rows is dropped — and the largest community of reorder.order_rabbit_device — a Cluster-GCN batch.
Per case: the count and fill kernels alone (the two C entry points on a prepared vertex map and row pointer, device events),
induced_subgraph as a whole with the construction of its CsrAdjacency and the first SpMM at k = 128 (wall clock: it
synchronises twice and the plan is built), and the same extraction in torch ops on the same GPU: the map gathered over every
entry of the selected rows, a mask, nonzero, a bincount and a cumsum, gathers — checked equal, integer for integer.
Also times random_walk (the set's size as roots, length 4).  The bytes the kernels must move are counted from the shapes
(every col entry of the touched rows once and a map word per entry, plus the outputs) and give an achieved rate.
Prints one JSON line and writes it to the profiles directory as subgraph_bench_reddit.json (--out FILE: elsewhere).

    python tools/subgraph_bench.py [--steps 20] [--warmup 5] [--scale 1.0] [--out FILE]
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
from gcn_amd import _lib, graphgen, reorder    # noqa: E402
from gcn_amd.spmm import _ptr, _stream_ptr    # noqa: E402


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


def torch_induced(adj, nodes, vmap):
    """the extraction in torch ops → (rowptr, col, eid) like the kernels' (the vertex map is the caller's, left cleared)"""
    ids = nodes.long()
    nn, dev = int(ids.numel()), ids.device
    vmap[ids] = torch.arange(nn, dtype=torch.int32, device=dev)
    rp = adj.rowptr.long()
    b, d = rp[ids], rp[ids + 1] - rp[ids]
    total = int(d.sum())
    starts = torch.cumsum(d, 0) - d
    rows = torch.repeat_interleave(torch.arange(nn, device=dev), d, output_size=total)
    e = b[rows] + torch.arange(total, device=dev) - starts[rows]
    loc = vmap[adj.col[e].long()]
    idx = (loc >= 0).nonzero().squeeze(1)
    out_rowptr = torch.zeros(nn + 1, dtype=torch.int32, device=dev)
    out_rowptr[1:] = torch.cumsum(torch.bincount(rows[idx], minlength=nn), 0)
    vmap[ids] = -1
    return out_rowptr, loc[idx], e[idx].to(torch.int32)


def measure(adj, nodes, name, x, steps, warmup):
    dev = nodes.device
    nn = int(nodes.numel())
    sub = gcn_amd.induced_subgraph(adj, nodes, values="gcn")
    n32 = nodes.to(torch.int32)
    vmap = torch.full((adj.n,), -1, dtype=torch.int32, device=dev)
    vmap[nodes.long()] = torch.arange(nn, dtype=torch.int32, device=dev)
    ws = torch.empty(_lib.SUBGRAPH_WS_BYTES, dtype=torch.uint8, device=dev)
    out_len = torch.zeros(nn, dtype=torch.int32, device=dev)
    out_col, out_eid = torch.empty_like(sub.adj.col), torch.empty_like(sub.eid)
    lib = _lib.load()

    def count():
        lib.gcn_induced_subgraph_count_csr(_ptr(adj.rowptr), _ptr(adj.col), adj.m, adj.nnz, _ptr(n32), nn, _ptr(vmap), _ptr(out_len),
                                           _ptr(ws), ws.numel(), _stream_ptr(dev))

    def fill():
        lib.gcn_induced_subgraph_fill_csr(_ptr(adj.rowptr), _ptr(adj.col), adj.m, adj.nnz, _ptr(n32), nn, _ptr(vmap),
                                          _ptr(sub.adj.rowptr), _ptr(out_col), _ptr(out_eid), _ptr(ws), ws.numel(), _stream_ptr(dev))

    def whole():
        s = gcn_amd.induced_subgraph(adj, nodes, values="gcn")
        return gcn_amd.spmm(s.adj, x[s.node_ids])

    lens = (adj.rowptr[nodes.long() + 1] - adj.rowptr[nodes.long()]).long()
    touched, kept = int(lens.sum()), int(sub.adj.nnz)
    row = {"set": name, "nodes": nn, "entries_in_touched_rows": touched, "longest_row": int(lens.max()),
           "rows_over_long_limit": int((lens > _lib.SAMPLE_LONG_ROW).sum()), "subgraph_entries": kept,
           "count_ms": events_ms(count, steps, warmup), "fill_ms": events_ms(fill, steps, warmup)}
    count(); fill()
    torch.cuda.synchronize()
    ref = torch_induced(adj, nodes, vmap.clone().fill_(-1))
    row["equals_torch"] = (bool(torch.equal(out_len, (sub.adj.rowptr[1:] - sub.adj.rowptr[:-1]))) and
                           all(bool(torch.equal(a, b)) for a, b in zip((sub.adj.rowptr, out_col, out_eid), ref)) and
                           bool(torch.equal(out_col, sub.adj.col)) and bool(torch.equal(out_eid, sub.eid)))
    row["count_plus_fill_ms"] = round(row["count_ms"] + row["fill_ms"], 4)
    # the least traffic of the two calls: col and a map word per touched entry, twice (count, fill), the rows' pointers, the outputs
    least = 2 * (8 * touched + 12 * nn) + 4 * nn + 8 * kept
    row["least_bytes"] = least
    row["count_plus_fill_gb_per_s"] = round(least / (row["count_plus_fill_ms"] * 1e-3) / 1e9, 1)
    row["induced_subgraph_ms"] = wall_ms(lambda: gcn_amd.induced_subgraph(adj, nodes, values="gcn"), steps, warmup)
    row["induced_subgraph_plan_spmm_k128_ms"] = wall_ms(whole, max(2, steps // 4), 1)
    few = max(2, min(steps, 5))
    tmap = torch.full((adj.n,), -1, dtype=torch.int32, device=dev)
    row["torch_induced_ms"] = wall_ms(lambda: torch_induced(adj, nodes, tmap), few, 1)
    row["torch_over_count_plus_fill"] = round(row["torch_induced_ms"] / row["count_plus_fill_ms"], 1)
    row["torch_over_induced_subgraph"] = round(row["torch_induced_ms"] / row["induced_subgraph_ms"], 2)
    roots = nodes[:min(nn, 20000)]
    row["random_walk_roots"] = int(roots.numel())
    row["random_walk_len4_ms"] = wall_ms(lambda: gcn_amd.random_walk(adj, roots, 4, seed=1, offset=0), steps, warmup)
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
    _, comm = reorder.order_rabbit_device(adj.rowptr, adj.col, return_communities=True)
    ids, sizes = torch.unique(comm.long(), return_counts=True)
    biggest = (comm.long() == ids[sizes.argmax()]).nonzero().squeeze(1)
    x = torch.randn((n, 128), device=dev)
    res = {"graph": "reddit", "scale": args.scale, "n": n, "nnz": adj.nnz, "steps": args.steps, "warmup": args.warmup,
           "long_row_limit": _lib.SAMPLE_LONG_ROW, "rabbit_communities": int(ids.numel()),
           "what": "ms per call; count_ms / fill_ms: device events around the C entry points alone; the others wall clock, host "
                   "synchronisations included; induced_subgraph_plan_spmm_k128_ms adds the CsrAdjacency's plan build and one "
                   "SpMM at k = 128; torch_induced_ms: the same extraction in torch ops",
           "cases": []}
    ok = True
    for name, nodes in (("random_2000", perm[:min(2000, n)]), ("random_20000", perm[:min(20000, n)]),
                        ("largest_rabbit_community", biggest)):
        row = measure(adj, nodes, name, x, args.steps, args.warmup)
        ok = ok and row["equals_torch"]
        res["cases"].append(row)
        print(f"# {row}", file=sys.stderr, flush=True)
    res["error_check"] = "pass" if ok else "FAIL"
    line = json.dumps(res)
    print(line)
    out = args.out or os.path.join(ROOT, "profiles", "subgraph_bench_reddit.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

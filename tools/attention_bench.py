#!/usr/bin/env python3
"""Attention aggregation on the headline graph (Reddit-shaped, graphgen.make_graph("reddit")): milliseconds of the edge
softmax forward and backward, of the fused GAT form forward and backward, and of one whole GraphAttention forward +
backward at k = 128 (heads = 1) — against two yardsticks that are not the code under test: `out.copy_(scores)` on an
nnz-float tensor (the same 2*4*nnz bytes the forward moves) and the stock-torch composition of the softmax
(torch.segment_reduce max / sum + repeat_interleave + exp + div), forward and backward, on the same scores.
CUDA events around `steps` calls after `warmup` calls.  Prints one JSON line; --out also writes it to a file.

    python tools/attention_bench.py [--steps 20] [--warmup 5] [--scale 1.0] [--k 128] [--no-stock] [--out FILE]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import gcn_amd                  # noqa: E402
from gcn_amd import graphgen    # noqa: E402


def time_ms(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) / steps, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--k", type=int, default=128)
    ap.add_argument("--no-stock", action="store_true", help="leave the stock-torch composition out (a kernel trace of ours alone)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rowptr, col, val, n = graphgen.make_graph("reddit", device=dev, seed=1, scale=args.scale)
    nnz = int(col.numel())
    lens = (rowptr[1:] - rowptr[:-1]).long()
    adj = gcn_amd.CsrAdjacency(rowptr, col, val, (n, n), symmetric=True, mutable_values=True)
    T = lambda fn: time_ms(fn, args.steps, args.warmup)
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    scores = (torch.rand(nnz, generator=gen, device=dev) * 16 - 8).requires_grad_(True)
    g = torch.randn(nnz, generator=gen, device=dev)
    res = {"graph": "reddit", "n": n, "nnz": nnz, "scale": args.scale, "steps": args.steps, "warmup": args.warmup,
           "max_row": int(lens.max()), "rows_over_8192": int((lens > 8192).sum()),
           "what": "ms per call, CUDA events around `steps` calls after `warmup` calls",
           "forward_bytes": 8 * nnz, "backward_bytes": 12 * nnz}

    # yardstick 1: a copy of nnz floats (reads 4 nnz, writes 4 nnz: what the forward has to move)
    out = torch.empty(nnz, device=dev)
    res["copy_ms"] = T(lambda: out.copy_(scores.detach()))

    # the edge softmax
    res["edge_softmax_fwd_ms"] = T(lambda: gcn_amd.edge_softmax(adj, scores.detach()))
    p = gcn_amd.edge_softmax(adj, scores)
    res["edge_softmax_bwd_ms"] = T(lambda: torch.autograd.grad(p, scores, g, retain_graph=True))
    res["edge_softmax_fwd_over_copy"] = round(res["edge_softmax_fwd_ms"] / res["copy_ms"], 3)
    res["edge_softmax_fwd_TBps"] = round(8 * nnz / res["edge_softmax_fwd_ms"] / 1e9, 3)
    res["edge_softmax_bwd_TBps"] = round(12 * nnz / res["edge_softmax_bwd_ms"] / 1e9, 3)

    # the fused GAT form (a_src: n floats, gathered)
    a_dst = (torch.rand(n, generator=gen, device=dev) * 8 - 4).requires_grad_(True)
    a_src = (torch.rand(n, generator=gen, device=dev) * 8 - 4).requires_grad_(True)
    res["gat_fwd_ms"] = T(lambda: gcn_amd.gat_edge_softmax(adj, a_dst.detach(), a_src.detach(), 0.2))
    pg = gcn_amd.gat_edge_softmax(adj, a_dst, a_src, 0.2)
    res["gat_bwd_ms"] = T(lambda: torch.autograd.grad(pg, (a_dst, a_src), g, retain_graph=True))
    res["gat_max_abs_diff_vs_unfused"] = float(
        (pg.detach() - gcn_amd.edge_softmax(adj, torch.nn.functional.leaky_relu(
            a_dst.detach().repeat_interleave(lens) + a_src.detach()[col.long()], 0.2))).abs().max())
    del p, pg

    # one whole layer, forward + backward
    k = args.k
    layer = gcn_amd.GraphAttention(k, k, heads=1).to(dev)
    x = torch.randn((n, k), generator=gen, device=dev, requires_grad=True)
    gout = torch.randn((n, k), generator=gen, device=dev)

    def layer_step():
        x.grad = None
        layer.zero_grad(set_to_none=True)
        layer(x, adj).backward(gout)
    res["graph_attention_fwd_bwd_ms"] = T(layer_step)
    res["graph_attention_k"] = k

    # yardstick 2: the same softmax composed from stock torch ops
    if not args.no_stock:
        try:
            def stock(s):
                mx = torch.segment_reduce(s, "max", lengths=lens)
                e = torch.exp(s - torch.repeat_interleave(mx, lens, output_size=nnz))
                return e / torch.repeat_interleave(torch.segment_reduce(e, "sum", lengths=lens), lens, output_size=nnz)
            res["stock_fwd_ms"] = T(lambda: stock(scores.detach()))
            ps = stock(scores)
            res["stock_bwd_ms"] = T(lambda: torch.autograd.grad(ps, scores, g, retain_graph=True))
            res["stock_max_abs_diff"] = float((ps.detach() - gcn_amd.edge_softmax(adj, scores.detach())).abs().max())
            res["stock_fwd_over_ours"] = round(res["stock_fwd_ms"] / res["edge_softmax_fwd_ms"], 2)
            res["stock_bwd_over_ours"] = round(res["stock_bwd_ms"] / res["edge_softmax_bwd_ms"], 2)
        except RuntimeError as e:                                            # (out of memory, unsupported op)
            res["stock_error"] = str(e)[:200]
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

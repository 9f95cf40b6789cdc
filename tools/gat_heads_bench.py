#!/usr/bin/env python3
"""All attention heads in one pass on the headline graph (Reddit-shaped, graphgen.make_graph("reddit")): milliseconds of
each head-batched kernel (gcn_amd/csrc/edge_softmax.hip, multihead.hip) at H heads x F columns, of one GraphAttention forward + backward
with head_batched=True and, in the same run, with the per-head loop (head_batched=False) — and three yardsticks that are
not the code under test: the weighted spmm(adj, x, values=) at the same k, and the single-head edge softmax and GAT
softmax whose time x H is what the per-head loop pays.
CUDA events around `steps` calls after `warmup` calls.  Prints one JSON line; --out also writes it to a file.

    python tools/gat_heads_bench.py [--steps 10] [--warmup 3] [--scale 1.0] [--heads 8] [--features 8,16] [--out FILE]
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


def one_shape(adj, madj, n, nnz, H, F, T, gen, dev):
    k = H * F
    res = {"heads": H, "features": F, "k": k}
    x = torch.randn((n, k), generator=gen, device=dev, requires_grad=True)
    gout = torch.randn((n, k), generator=gen, device=dev)
    scores = (torch.rand((nnz, H), generator=gen, device=dev) * 16 - 8).requires_grad_(True)
    gp = torch.randn((nnz, H), generator=gen, device=dev)
    a_dst = (torch.rand((n, H), generator=gen, device=dev) * 8 - 4).requires_grad_(True)
    a_src = (torch.rand((n, H), generator=gen, device=dev) * 8 - 4).requires_grad_(True)

    # the new kernels, one at a time
    res["edge_softmax_heads_fwd_ms"] = T(lambda: gcn_amd.edge_softmax(adj, scores.detach()))
    p = gcn_amd.edge_softmax(adj, scores)
    res["edge_softmax_heads_bwd_ms"] = T(lambda: torch.autograd.grad(p, scores, gp, retain_graph=True))
    res["gat_heads_fwd_ms"] = T(lambda: gcn_amd.gat_edge_softmax(adj, a_dst.detach(), a_src.detach(), 0.2))
    pg = gcn_amd.gat_edge_softmax(adj, a_dst, a_src, 0.2)
    res["gat_heads_bwd_ms"] = T(lambda: torch.autograd.grad(pg, (a_dst, a_src), gp, retain_graph=True))
    trp, _trow, tperm = adj.tpattern()      # (grad_a_src: the segment sum inside the line above)
    res["segment_sum_heads_transposed_ms"] = T(lambda: gcn_amd.segment_sum(trp, gp, perm=tperm))
    res["segment_sum_heads_ms"] = T(lambda: gcn_amd.segment_sum(adj.rowptr, gp))
    pv = p.detach().clone().requires_grad_(True)
    res["spmm_heads_fwd_ms"] = T(lambda: gcn_amd.spmm_heads(adj, x.detach(), pv.detach()))
    out = gcn_amd.spmm_heads(adj, x, pv)
    res["spmm_heads_transposed_ms"] = T(lambda: torch.autograd.grad(out, x, gout, retain_graph=True))
    res["sddmm_heads_ms"] = T(lambda: gcn_amd.sddmm_heads(adj, gout, x.detach(), H))
    del out, pg

    # yardsticks: the single-head units the loop is made of, and the weighted SpMM at the same k
    s1 = scores.detach()[:, 0].contiguous()
    res["edge_softmax_1head_fwd_ms"] = T(lambda: gcn_amd.edge_softmax(madj, s1))
    ad1, as1 = a_dst.detach()[:, 0].contiguous(), a_src.detach()[:, 0].contiguous()
    res["gat_1head_fwd_ms"] = T(lambda: gcn_amd.gat_edge_softmax(madj, ad1, as1, 0.2))
    p1 = p.detach()[:, 0].contiguous()
    res["spmm_values_same_k_ms"] = T(lambda: gcn_amd.spmm(madj, x.detach(), values=p1))
    xf = x.detach()[:, :F].contiguous()
    res["spmm_values_one_head_ms"] = T(lambda: gcn_amd.spmm(madj, xf, values=p1))
    res["edge_softmax_heads_fwd_over_1head_x_H"] = round(res["edge_softmax_heads_fwd_ms"] / (H * res["edge_softmax_1head_fwd_ms"]), 3)
    res["gat_heads_fwd_over_1head_x_H"] = round(res["gat_heads_fwd_ms"] / (H * res["gat_1head_fwd_ms"]), 3)
    res["spmm_heads_fwd_over_one_head_x_H"] = round(res["spmm_heads_fwd_ms"] / (H * res["spmm_values_one_head_ms"]), 3)
    res["spmm_heads_fwd_over_spmm_values_same_k"] = round(res["spmm_heads_fwd_ms"] / res["spmm_values_same_k_ms"], 3)
    del p, pv, p1

    # the layer: forward + backward, head-batched and the loop, same parameters
    torch.manual_seed(0)
    loop = gcn_amd.GraphAttention(k, F, heads=H).to(dev)
    batched = gcn_amd.GraphAttention(k, F, heads=H, head_batched=True).to(dev)
    batched.load_state_dict(loop.state_dict())

    def step(layer, a):
        def run():
            x.grad = None
            layer.zero_grad(set_to_none=True)
            layer(x, a).backward(gout)
        return run
    res["graph_attention_batched_fwd_bwd_ms"] = T(step(batched, adj))
    res["graph_attention_loop_fwd_bwd_ms"] = T(step(loop, madj))
    res["loop_over_batched"] = round(res["graph_attention_loop_fwd_bwd_ms"] / res["graph_attention_batched_fwd_bwd_ms"], 2)
    with torch.no_grad():
        ob, ol = batched(x, adj), loop(x, madj)
        res["batched_vs_loop_max_abs_diff"] = float((ob - ol).abs().max())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--heads", type=int, default=8)
    ap.add_argument("--features", default="8,16", help="columns per head, comma-separated")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rowptr, col, val, n = graphgen.make_graph("reddit", device=dev, seed=1, scale=args.scale)
    nnz = int(col.numel())
    lens = (rowptr[1:] - rowptr[:-1]).long()
    adj = gcn_amd.CsrAdjacency(rowptr, col, val, (n, n), symmetric=True)                          # the head-batched path: no plan
    madj = gcn_amd.CsrAdjacency(rowptr, col, val, (n, n), symmetric=True, mutable_values=True)    # the loop's mutable plan
    T = lambda fn: time_ms(fn, args.steps, args.warmup)
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    res = {"graph": "reddit", "n": n, "nnz": nnz, "scale": args.scale, "steps": args.steps, "warmup": args.warmup,
           "max_row": int(lens.max()), "mean_row": round(nnz / max(n, 1), 1),
           "what": "ms per call, CUDA events around `steps` calls after `warmup` calls", "shapes": []}
    for F in (int(f) for f in args.features.split(",")):
        res["shapes"].append(one_shape(adj, madj, n, nnz, args.heads, F, T, gen, dev))
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

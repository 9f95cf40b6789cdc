#!/usr/bin/env python3
"""Learnable edge weights on the headline graph (Reddit-shaped, graphgen.make_graph("reddit")): SDDMM milliseconds at
k = 64 / 128 / 256 with the kernel each call launches and its error on sampled entries against fp64
(|d - d*| <= 1e-5 sum_j |A_rj B_cj|, reported as the largest ratio error / bound; <= 1 passes); update_values for the
adjacency and its transpose; one learnable-weight SpMM forward + backward against the fixed-weight (weighted) SpMM
forward + backward at the same k; and, for context, stock torch.sparse.mm forward + backward with a grad-requiring COO
operand on a scaled-down graph.  Prints one JSON line.

    python tools/sddmm_bench.py [--steps 20] [--warmup 5] [--ks 64,128,256] [--scale 1.0] [--stock-scale 0.1]
"""
import argparse
import json
import os
import sys

import numpy as np
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


def bound_ratio(rowptr, col, A, B, out, sample):
    """max over sampled entries of |d - d*| / (1e-5 sum_j |A_rj B_cj| + 1e-30)"""
    dev = out.device
    e = torch.from_numpy(sample).to(dev)
    rows = torch.searchsorted(rowptr.long(), e, right=True) - 1
    p = A[rows].double() * B[col[e].long()].double()
    ref, mag = p.sum(1), p.abs().sum(1)
    return float(((out[e].double() - ref).abs() / (1e-5 * mag + 1e-30)).max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--ks", default="64,128,256")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--stock-scale", type=float, default=0.1)
    ap.add_argument("--sample", type=int, default=200000)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rowptr, col, val, n = graphgen.make_graph("reddit", device=dev, seed=1, scale=args.scale)
    nnz = int(col.numel())
    sample = np.sort(np.random.default_rng(0).choice(nnz, min(args.sample, nnz), replace=False))
    fixed = gcn_amd.CsrAdjacency(rowptr, col, val, (n, n), symmetric=True)
    fixed.plan                                                           # noqa: B018  (builds the plan)
    fixed.set_value_factors(None, None)                                  # the weighted pass, as bench.py's weighted leg
    adj = gcn_amd.CsrAdjacency(rowptr, col, val, (n, n), symmetric=True, mutable_values=True)
    res = {"graph": "reddit", "n": n, "nnz": nnz, "scale": args.scale, "steps": args.steps, "warmup": args.warmup,
           "slices_mutable": adj.num_slices, "slices_fixed_weighted": fixed.num_slices,
           "what": "ms per call, CUDA events around `steps` calls", "sddmm": [], "train": []}
    w = val.clone().requires_grad_(True)
    adjT = adj.transpose()
    wT = w.detach().index_select(0, adj.tpattern()[2])
    res["update_values_ms"] = time_ms(lambda: adj.update_values(w), args.steps, args.warmup)
    res["update_values_transpose_ms"] = time_ms(lambda: adjT.update_values(wT), args.steps, args.warmup)
    ok = True
    for k in [int(x) for x in args.ks.split(",")]:
        g = torch.Generator(device=dev)
        g.manual_seed(k)
        A = torch.randn((n, k), generator=g, device=dev)
        B = torch.randn((n, k), generator=g, device=dev)
        out = torch.empty(nnz, device=dev)
        row = {"k": k, "sddmm_ms": time_ms(lambda: adj.sddmm(A, B, out=out), args.steps, args.warmup),
               "sddmm_kernel": adj.sddmm_kernel(k),
               "weighted_spmm_ms": time_ms(lambda: fixed.matmul_raw(B), args.steps, args.warmup),
               "weighted_spmm_kernel": fixed.main_kernel(k)}
        row["bound_ratio"] = round(bound_ratio(rowptr, col, A, B, out, sample), 4)
        row["sddmm_over_weighted_spmm"] = round(row["sddmm_ms"] / row["weighted_spmm_ms"], 3)
        ok = ok and row["bound_ratio"] <= 1.0
        res["sddmm"].append(row)
        print(f"# {row}", file=sys.stderr, flush=True)
        if k == 128:
            X = B.clone().requires_grad_(True)
            gout = torch.randn((n, k), generator=g, device=dev)

            def learnable():
                w.grad = X.grad = None
                gcn_amd.spmm(adj, X, values=w).backward(gout)

            def weighted():
                X.grad = None
                gcn_amd.spmm(fixed, X).backward(gout)
            t = {"k": k, "learnable_fwd_bwd_ms": time_ms(learnable, args.steps, args.warmup),
                 "fixed_weighted_fwd_bwd_ms": time_ms(weighted, args.steps, args.warmup)}
            res["train"].append(t)
            print(f"# {t}", file=sys.stderr, flush=True)
        del A, B, out
    # stock PyTorch for context, on a scaled-down graph (its COO backward materialises per-entry products);
    # --stock-scale 0 leaves it out (a kernel trace of the headline graph alone)
    try:
        if args.stock_scale <= 0:
            raise RuntimeError("left out (--stock-scale 0)")
        rp_s, col_s, val_s, n_s = graphgen.make_graph("reddit", device=dev, seed=1, scale=args.stock_scale)
        rows_s = torch.repeat_interleave(torch.arange(n_s, device=dev), rp_s.long()[1:] - rp_s.long()[:-1])
        idx = torch.stack([rows_s, col_s.long()])
        k = 128
        X = torch.randn((n_s, k), device=dev, requires_grad=True)
        gout = torch.randn((n_s, k), device=dev)
        a = torch.sparse_coo_tensor(idx, val_s, (n_s, n_s)).coalesce().requires_grad_(True)

        def stock():
            a.grad = X.grad = None
            torch.sparse.mm(a, X).backward(gout)
        adj_s = gcn_amd.CsrAdjacency(rp_s, col_s, val_s, (n_s, n_s), mutable_values=True)
        w_s = val_s.clone().requires_grad_(True)

        def ours():
            w_s.grad = X.grad = None
            gcn_amd.spmm(adj_s, X, values=w_s).backward(gout)
        res["stock_context"] = {"scale": args.stock_scale, "n": n_s, "nnz": int(col_s.numel()), "k": k,
                                "torch_sparse_mm_fwd_bwd_ms": time_ms(stock, 5, 2),
                                "learnable_fwd_bwd_ms": time_ms(ours, args.steps, args.warmup)}
    except RuntimeError as e:                                            # (out of memory, unsupported op)
        res["stock_context"] = {"error": str(e)[:200]}
    res["error_check"] = "pass" if ok else "FAIL"
    print(json.dumps(res))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

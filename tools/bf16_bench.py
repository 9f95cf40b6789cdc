#!/usr/bin/env python3
"""bf16 feature operands against fp32 on the headline graph (Reddit-shaped, graphgen.make_graph("reddit")): whole-SpMM
milliseconds for fp32, bf16 -> fp32 and bf16 -> bf16, value-free and weighted (a second plan told to forget the value
factors, as bench.py's weighted leg), at k = 128 and 256, with the main kernel each call launches and the error of
sampled rows against an fp64 evaluation (elementwise bound of DESIGN.md §bf16: |C - C*| <= 2^-8 |A||B| + 2^-8 |C*| + 1e-6,
reported as the largest ratio error / bound; <= 1 passes).  Prints one JSON line.

    python tools/bf16_bench.py [--steps 20] [--warmup 5] [--ks 128,256] [--scale 1.0]
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


def bound_ratio(rowptr, col, val, B, C, rows, bf16_out):
    """max over sampled rows of |C - C*| / bound, C* and |A||B| in fp64 on the device"""
    dev = C.device
    r = torch.from_numpy(rows).to(dev)
    rp = rowptr.long()
    start, lens = rp[r], rp[r + 1] - rp[r]
    seg = torch.repeat_interleave(torch.arange(len(rows), device=dev), lens)
    first = torch.cumsum(lens, 0) - lens
    e = start[seg] + (torch.arange(int(lens.sum()), device=dev) - first[seg])
    v, cc = val[e].double(), col[e].long()
    Bd = B[cc].double()
    ref = torch.zeros((len(rows), B.shape[1]), dtype=torch.float64, device=dev).index_add_(0, seg, v[:, None] * Bd)
    mag = torch.zeros_like(ref).index_add_(0, seg, v.abs()[:, None] * Bd.abs())
    bound = 2.0 ** -8 * mag + (2.0 ** -8 * ref.abs() if bf16_out else 0.0) + 1e-6
    return float(((C[r].double() - ref).abs() / bound).max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--ks", default="128,256")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--sample", type=int, default=2000)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rowptr, col, val, n = graphgen.make_graph("reddit", device=dev, seed=1, scale=args.scale)
    nnz = int(col.numel())
    rows = np.sort(np.random.default_rng(0).choice(n, min(args.sample, n), replace=False))
    plans = {"value_free": gcn_amd.CsrAdjacency(rowptr, col, val, (n, n), symmetric=True)}
    w = gcn_amd.CsrAdjacency(rowptr, col, val, (n, n), symmetric=True)
    w.plan                                                               # noqa: B018  (builds the plan)
    w.set_value_factors(None, None)
    plans["weighted"] = w
    res = {"graph": "reddit", "n": n, "nnz": nnz, "scale": args.scale, "steps": args.steps, "warmup": args.warmup,
           "what": "ms per whole SpMM (re-lay of B, main kernel, slice reduction), CUDA events around `steps` calls",
           "results": []}
    for k in [int(x) for x in args.ks.split(",")]:
        g = torch.Generator(device=dev)
        g.manual_seed(k)
        B32 = torch.randn((n, k), generator=g, device=dev, dtype=torch.float32)
        B16 = B32.to(torch.bfloat16)
        B16up = B16.float()
        o32 = torch.empty((n, k), dtype=torch.float32, device=dev)
        o16 = torch.empty((n, k), dtype=torch.bfloat16, device=dev)
        for pname, adj in plans.items():
            row = {"k": k, "pass": pname}
            row["fp32_ms"] = time_ms(lambda: adj.matmul_raw(B32, out=o32), args.steps, args.warmup)
            row["fp32_kernel"] = adj.main_kernel(k)
            row["bf16_to_fp32_ms"] = time_ms(lambda: adj.matmul_raw(B16, out=o32), args.steps, args.warmup)
            row["bf16_to_fp32_bound_ratio"] = round(bound_ratio(rowptr, col, val, B16up, o32, rows, False), 4)
            row["bf16_to_bf16_ms"] = time_ms(lambda: adj.matmul_raw(B16, out=o16), args.steps, args.warmup)
            row["bf16_to_bf16_bound_ratio"] = round(bound_ratio(rowptr, col, val, B16up, o16, rows, True), 4)
            row["bf16_kernel"] = adj.main_kernel(k, dtype=torch.bfloat16)
            res["results"].append(row)
            print(f"# {row}", file=sys.stderr, flush=True)
        del B32, B16, B16up, o32, o16
    ok = all(r["bf16_to_fp32_bound_ratio"] <= 1.0 and r["bf16_to_bf16_bound_ratio"] <= 1.0 for r in res["results"])
    res["error_check"] = "pass" if ok else "FAIL"
    print(json.dumps(res))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Max aggregation (gcn_amd.aggregate, gcn_amd/csrc/aggregate.hip) on the headline graph (Reddit-shaped,
graphgen.make_graph("reddit")) at k = 128, fp32 and bf16: forward and backward milliseconds against two yardsticks —
the value-free sum SpMM of the same adjacency (gcn_amd.spmm forward, its transpose product as the backward), and, on a
scaled-down graph where its nnz x k intermediate fits, the stock formulation x[col] + torch.segment_reduce("max") and its
autograd backward.  Each row carries the bytes model of DESIGN §4.11 (gathered rows + out + arg; backward: gathered g and
arg rows + gx) and the rate it implies.  The forward is checked against torch's result on the scaled graph (equal values).
Prints one JSON line and writes it to the profiles directory as aggregate_bench_reddit_k<k>.json (--out FILE: elsewhere).

    python tools/aggregate_bench.py [--steps 20] [--warmup 5] [--k 128] [--scale 1.0] [--stock-scale 0.1] [--out FILE]
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


def bytes_model(m, n, nnz, k, esize):
    """bytes one call needs (every gathered row counted: most of them come from L2, not HBM)"""
    fwd = nnz * (k * esize + 4) + m * k * (esize + 4) + 4 * (m + 1)
    bwd = nnz * (k * (esize + 4) + 8) + n * k * esize + 4 * (n + 1)
    spmm = nnz * (k * esize + 4) + m * k * esize + 4 * (m + 1)
    return fwd, bwd, spmm


def measure(rowptr, col, val, n, k, dtype, steps, warmup, stock):
    dev = col.device
    nnz = int(col.numel())
    adj = gcn_amd.CsrAdjacency(rowptr, col, val, (n, n), symmetric=True)
    esize = 2 if dtype == torch.bfloat16 else 4
    g = torch.Generator(device=dev)
    g.manual_seed(k)
    x = torch.randn((n, k), generator=g, device=dev).to(dtype).requires_grad_(True)
    gout = torch.randn((n, k), generator=g, device=dev).to(dtype)
    out, arg = gcn_amd.aggregate(adj, x, "max", return_arg=True)
    fwd_b, bwd_b, spmm_b = bytes_model(n, n, nnz, k, esize)
    row = {"dtype": str(dtype).replace("torch.", ""), "k": k, "n": n, "nnz": nnz,
           "max_fwd_ms": time_ms(lambda: gcn_amd.aggregate(adj, x.detach(), "max"), steps, warmup),
           "max_bwd_ms": time_ms(lambda: torch.autograd.grad(out, x, gout, retain_graph=True), steps, warmup),
           "sum_spmm_fwd_ms": time_ms(lambda: adj.matmul_raw(x.detach()), steps, warmup),
           "sum_spmm_bwd_ms": time_ms(lambda: adj.transpose().matmul_raw(gout), steps, warmup),
           "sum_spmm_kernel": adj.main_kernel(k, dtype=dtype),
           "model_bytes": {"max_fwd": fwd_b, "max_bwd": bwd_b, "sum_spmm": spmm_b}}
    row["max_fwd_over_sum_spmm"] = round(row["max_fwd_ms"] / row["sum_spmm_fwd_ms"], 3)
    row["max_bwd_over_sum_spmm"] = round(row["max_bwd_ms"] / row["sum_spmm_bwd_ms"], 3)
    row["model_fwd_over_sum_spmm"] = round(fwd_b / spmm_b, 3)
    row["max_fwd_model_TBps"] = round(fwd_b / row["max_fwd_ms"] / 1e9, 3)
    row["max_bwd_model_TBps"] = round(bwd_b / row["max_bwd_ms"] / 1e9, 3)
    if stock:
        try:
            lens = (rowptr.long()[1:] - rowptr.long()[:-1])
            xs = x.detach().float().requires_grad_(True)
            cl = col.long()

            def stock_fwd():
                return torch.segment_reduce(xs[cl], "max", lengths=lens)
            ref = stock_fwd()
            row["torch_fwd_ms"] = time_ms(lambda: stock_fwd(), min(steps, 5), 2)
            row["torch_bwd_ms"] = time_ms(lambda: torch.autograd.grad(ref, xs, gout.float(), retain_graph=True), min(steps, 5), 2)
            row["torch_fwd_over_max_fwd"] = round(row["torch_fwd_ms"] / row["max_fwd_ms"], 3)
            row["torch_bwd_over_max_bwd"] = round(row["torch_bwd_ms"] / row["max_bwd_ms"], 3)
            row["torch_min_bytes"] = 3 * nnz * k * 4
            nonempty = (lens > 0)[:, None]
            row["equals_torch"] = bool(torch.equal(torch.where(nonempty, out.detach().float(), ref.detach()), ref.detach()))
        except RuntimeError as e:                                        # (out of memory, unsupported op)
            row["torch_error"] = str(e)[:200]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--k", type=int, default=128)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--stock-scale", type=float, default=0.1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"graph": "reddit", "steps": args.steps, "warmup": args.warmup,
           "what": "ms per call, CUDA events around `steps` calls; model_bytes: what one call needs, gathered rows included",
           "full": [], "scaled": []}
    ok = True
    for scale, key, stock in ((args.scale, "full", False), (args.stock_scale, "scaled", True)):
        if scale <= 0:
            continue
        rowptr, col, val, n = graphgen.make_graph("reddit", device=dev, seed=1, scale=scale)
        for dtype in (torch.float32, torch.bfloat16):
            row = measure(rowptr, col, val, n, args.k, dtype, args.steps, args.warmup, stock and dtype == torch.float32)
            row["scale"] = scale
            ok = ok and row.get("equals_torch", True)
            res[key].append(row)
            print(f"# {row}", file=sys.stderr, flush=True)
        del rowptr, col, val
        torch.cuda.empty_cache()
    res["error_check"] = "pass" if ok else "FAIL"
    line = json.dumps(res)
    print(line)
    out = args.out or os.path.join(ROOT, "profiles", f"aggregate_bench_reddit_k{args.k}.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Edge-feature aggregation (gcn_amd.edge_aggregate, gcn_amd/csrc/edge_message.hip) on the Reddit-shaped graph
(graphgen.make_graph("reddit")) at --scale (default 0.25: 28.7 M entries, so that edge_feat at k = 64 has 7.3 GB and the
torch formulation's three [nnz, k] intermediates fit beside it; the scale is recorded), k in {16, 64}: milliseconds of the
forward and of forward + backward (gradients in x and in edge_feat) for ``add + relu + sum`` (GINE's message) and
``mul + max``, and in the same run
  * the torch formulation: (x[col] op w).relu() reduced with index_add_ / scatter_reduce, and its autograd backward;
  * the yardsticks of the gather walk alone at the same k: aggregate(adj, x, "max") and spmm_heads with one head;
  * the byte model of DESIGN §4.30: edge_feat streamed once, a gathered row of x per entry, the index words, out (and arg)
    — and for the backward g gathered per entry, edge_feat streamed twice, the gradient in edge_feat written once — divided
    by the measured copy bandwidth of the chip (6.29 TB/s, float4 copy), and the fraction of it each time reaches.
Times are CUDA events around `steps` calls after `warmup` calls.  The forward is checked against the torch formulation (sum:
the standing bound; max: equal values).  Prints one JSON line and writes it to profiles/edge_aggregate_bench.json.

    python tools/edge_aggregate_bench.py [--steps 20] [--warmup 5] [--scale 0.25] [--out FILE]
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

COPY_TBPS = 6.29                # measured float4 copy bandwidth of the MI355X
CONFIGS = [("add", "relu", "sum"), ("mul", None, "max")]


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


def bytes_model(m, n, nnz, k, reduce):
    """bytes one call needs (every gathered row counted, though most come from L2): forward, and forward + backward"""
    fwd = nnz * (2 * k * 4 + 4) + m * k * 4 * (2 if reduce == "max" else 1) + 4 * (m + 1)
    if reduce == "sum":
        bwd_x = nnz * (2 * k * 4 + 8) + 2 * n * k * 4 + 4 * (n + 1)       # g gathered, w by permutation, x's own row, gx
        bwd_e = nnz * (3 * k * 4 + 4) + m * k * 4 + 4 * (m + 1)           # x gathered, w read, ge written, g per row
    else:                                                                 # element-wise [m, k] work, a selection's backward
        bwd_x = nnz * 8 + m * k * 4 * 8 + n * k * 4
        bwd_e = nnz * k * 4 + m * k * 4 * 3                               # the zero fill of ge and the scattered winners
    return fwd, fwd + bwd_x + bwd_e


def torch_formulation(rows, col, m, x, w, op, act, reduce):
    msg = x[col] * w if op == "mul" else x[col] + w
    if act == "relu":
        msg = msg.relu()
    k = x.shape[1]
    if reduce == "sum":
        return torch.zeros(m, k, device=x.device).index_add_(0, rows, msg)
    return torch.zeros(m, k, device=x.device).scatter_reduce(0, rows[:, None].expand(-1, k), msg, "amax", include_self=False)


def measure(adj, rows, col, k, steps, warmup):
    dev = adj.device
    m, n, nnz = adj.m, adj.n, adj.nnz
    gen = torch.Generator(device=dev)
    gen.manual_seed(k)
    x = torch.randn((n, k), generator=gen, device=dev).requires_grad_(True)
    w = torch.randn((nnz, k), generator=gen, device=dev).requires_grad_(True)
    gout = torch.randn((m, k), generator=gen, device=dev)
    out = {"k": k, "edge_feat_GB": round(nnz * k * 4 / 1e9, 3), "route_vec_lps_tiles": list(gcn_amd.edgefeat.route(k, x, w)), "configs": []}
    ok = True
    for op, act, reduce in CONFIGS:
        def fwd():
            return gcn_amd.edge_aggregate(adj, x.detach(), w.detach(), op, act, reduce)

        def fwd_bwd():
            return torch.autograd.grad(gcn_amd.edge_aggregate(adj, x, w, op, act, reduce), (x, w), gout)

        def t_fwd():
            with torch.no_grad():
                return torch_formulation(rows, col, m, x, w, op, act, reduce)

        def t_fwd_bwd():
            return torch.autograd.grad(torch_formulation(rows, col, m, x, w, op, act, reduce), (x, w), gout)

        fb, fbb = bytes_model(m, n, nnz, k, reduce)
        row = {"op": op, "act": act, "reduce": reduce, "fwd_ms": time_ms(fwd, steps, warmup), "fwd_bwd_ms": time_ms(fwd_bwd, steps, warmup),
               "model_bytes_fwd": fb, "model_bytes_fwd_bwd": fbb,
               "model_fwd_ms": round(fb / COPY_TBPS / 1e9, 4), "model_fwd_bwd_ms": round(fbb / COPY_TBPS / 1e9, 4)}
        row["fwd_fraction_of_model"] = round(row["model_fwd_ms"] / row["fwd_ms"], 3)
        row["fwd_bwd_fraction_of_model"] = round(row["model_fwd_bwd_ms"] / row["fwd_bwd_ms"], 3)
        try:
            ref = t_fwd()
            got = fwd()
            if reduce == "sum":
                with torch.no_grad():
                    mag = torch_formulation(rows, col, m, x.abs(), w.abs(), op, None, "sum")
                row["max_error_over_bound"] = round(float(((got - ref).abs() / (1e-5 * mag + 1e-30)).max()), 4)
                ok = ok and row["max_error_over_bound"] <= 1.0
            else:
                row["equals_torch"] = bool(torch.equal(got, ref))
                ok = ok and row["equals_torch"]
            del ref, got
            row["torch_fwd_ms"] = time_ms(t_fwd, min(steps, 5), 2)
            row["torch_fwd_bwd_ms"] = time_ms(t_fwd_bwd, min(steps, 5), 2)
            row["torch_fwd_over_fwd"] = round(row["torch_fwd_ms"] / row["fwd_ms"], 3)
            row["torch_fwd_bwd_over_fwd_bwd"] = round(row["torch_fwd_bwd_ms"] / row["fwd_bwd_ms"], 3)
        except RuntimeError as e:                                        # (out of memory, unsupported op)
            row["torch_error"] = str(e)[:200]
        out["configs"].append(row)
        print(f"# k={k} {row}", file=sys.stderr, flush=True)
        torch.cuda.empty_cache()
    xd = x.detach()
    ones = torch.ones((nnz, 1), device=dev)
    out["yardsticks"] = {"aggregate_max_fwd_ms": time_ms(lambda: gcn_amd.aggregate(adj, xd, "max"), steps, warmup),
                         "spmm_heads_H1_fwd_ms": time_ms(lambda: gcn_amd.spmm_heads(adj, xd, ones), steps, warmup),
                         "gather_walk_bytes": nnz * (k * 4 + 4) + m * k * 4 + 4 * (m + 1)}
    out["yardsticks"]["gather_walk_model_ms"] = round(out["yardsticks"]["gather_walk_bytes"] / COPY_TBPS / 1e9, 4)
    print(f"# k={k} {out['yardsticks']}", file=sys.stderr, flush=True)
    return out, ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--scale", type=float, default=0.25)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("edge_aggregate_bench: no GPU (there is no CPU path and nothing to time without one)", file=sys.stderr)
        return 2
    dev = torch.device("cuda:0")
    rowptr, col, val, n = graphgen.make_graph("reddit", device=dev, seed=1, scale=args.scale)
    adj = gcn_amd.CsrAdjacency(rowptr, col, val, (n, n), symmetric=True)
    lens = rowptr.long()[1:] - rowptr.long()[:-1]
    rows = torch.repeat_interleave(torch.arange(n, device=dev), lens)
    res = {"graph": "reddit", "scale": args.scale, "n": n, "nnz": adj.nnz, "steps": args.steps, "warmup": args.warmup,
           "copy_TBps": COPY_TBPS, "device": torch.cuda.get_device_name(dev),
           "what": "ms per call, CUDA events around `steps` calls; model: the bytes one call needs over the copy bandwidth",
           "widths": []}
    ok = True
    for k in (16, 64):
        row, good = measure(adj, rows, col.long(), k, args.steps, args.warmup)
        res["widths"].append(row)
        ok = ok and good
    res["error_check"] = "pass" if ok else "FAIL"
    line = json.dumps(res)
    print(line)
    out = args.out or os.path.join(ROOT, "profiles", "edge_aggregate_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""GATv2 scores on the headline graph (Reddit-shaped, graphgen.make_graph("reddit")): milliseconds of gatv2_scores forward,
of each of its two backward walks and of its forward + backward through autograd (gcn_amd/csrc/multihead.hip) at H heads x F
columns, of one GraphAttentionV2 forward + backward — and, in the same process, what they are measured against: sddmm_heads
and spmm_heads (forward and transposed) at the same (H, F), whose gathers are the same bytes, and the torch formulation

    (leaky_relu(h_dst[row] + h_src[col]).view(nnz, H, F) * att).sum(-1)

with autograd, which materialises [nnz, H*F] tensors (where it does not fit in memory its entry says so: rerun everything
at a smaller --scale).  CUDA events around `steps` calls after `warmup` calls; the variants alternate for `--rounds`
rounds, every round's figure is kept, so the spread shows.  Prints one JSON line; --out also writes it to a file.

    python tools/gatv2_bench.py [--steps 10] [--warmup 3] [--rounds 2] [--scale 1.0] [--heads 8] [--features 8,16] [--out FILE]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F_

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import gcn_amd                  # noqa: E402
from gcn_amd import attention, graphgen    # noqa: E402


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


def one_shape(adj, n, nnz, H, F, T, rounds, gen, dev, with_torch):
    k = H * F
    res = {"heads": H, "features": F, "k": k}
    h_dst = torch.randn((n, k), generator=gen, device=dev, requires_grad=True)
    h_src = torch.randn((n, k), generator=gen, device=dev, requires_grad=True)
    att = torch.randn((H, F), generator=gen, device=dev, requires_grad=True)
    g = torch.randn((nnz, H), generator=gen, device=dev)
    gout = torch.randn((n, k), generator=gen, device=dev)
    vals = torch.rand((nnz, H), generator=gen, device=dev)
    hd, hs, a = h_dst.detach(), h_src.detach(), att.detach()
    trp, trow, tperm = adj.tpattern()
    row = torch.repeat_interleave(torch.arange(n, device=dev), (adj.rowptr[1:] - adj.rowptr[:-1]).long())
    col = adj.col.long()

    def fwd_bwd():
        h_dst.grad = h_src.grad = att.grad = None
        gcn_amd.gatv2_scores(adj, h_dst, h_src, att, 0.2).backward(g)

    def torch_fwd_bwd():
        h_dst.grad = h_src.grad = att.grad = None
        ((F_.leaky_relu(h_dst[row] + h_src[col], 0.2).view(nnz, H, F) * att).sum(-1)).backward(g)

    xs = h_src.detach().clone().requires_grad_(True)
    out = gcn_amd.spmm_heads(adj, xs, vals)
    torch.manual_seed(0)
    layer = gcn_amd.GraphAttentionV2(k, F, heads=H).to(dev)
    x = torch.randn((n, k), generator=gen, device=dev, requires_grad=True)

    def layer_step():
        x.grad = None
        layer.zero_grad(set_to_none=True)
        layer(x, adj).backward(gout)

    variants = [
        ("gatv2_scores_fwd_ms", lambda: gcn_amd.gatv2_scores(adj, hd, hs, a, 0.2)),
        ("gatv2_backward_pattern_ms", lambda: attention._gatv2_backward_raw(adj, adj.rowptr, adj.col, None, n, hd, hs, a, 0.2, g, True)),
        ("gatv2_backward_transposed_ms", lambda: attention._gatv2_backward_raw(adj, trp, trow, tperm, n, hs, hd, a, 0.2, g, False)),
        ("gatv2_scores_fwd_bwd_ms", fwd_bwd),
        ("sddmm_heads_ms", lambda: gcn_amd.sddmm_heads(adj, hd, hs, H)),
        ("spmm_heads_fwd_ms", lambda: gcn_amd.spmm_heads(adj, hs, vals)),
        ("spmm_heads_transposed_ms", lambda: torch.autograd.grad(out, xs, gout, retain_graph=True)),
        ("graph_attention_v2_fwd_bwd_ms", layer_step),
    ]
    if with_torch:
        variants.append(("torch_formulation_fwd_bwd_ms", torch_fwd_bwd))
    for name, _fn in variants:
        res[name] = []
    for _round in range(rounds):                            # the variants alternate: one figure each per round
        for name, fn in variants:
            if res[name] == "out of memory":
                continue
            try:
                res[name].append(T(fn))
            except torch.cuda.OutOfMemoryError:
                res[name] = "out of memory"
                torch.cuda.empty_cache()
    best = lambda name: min(res[name]) if isinstance(res[name], list) and res[name] else None
    res["gatv2_fwd_over_sddmm_heads"] = round(best("gatv2_scores_fwd_ms") / best("sddmm_heads_ms"), 3)
    res["gatv2_backward_pattern_over_spmm_heads_fwd"] = round(best("gatv2_backward_pattern_ms") / best("spmm_heads_fwd_ms"), 3)
    res["gatv2_backward_transposed_over_spmm_heads_transposed"] = round(
        best("gatv2_backward_transposed_ms") / best("spmm_heads_transposed_ms"), 3)
    if with_torch and best("torch_formulation_fwd_bwd_ms") is not None:
        # the slowest kernel round against the fastest torch round: the margin left after the run-to-run spread
        res["torch_over_gatv2_fwd_bwd_worst_case"] = round(min(res["torch_formulation_fwd_bwd_ms"]) / max(res["gatv2_scores_fwd_bwd_ms"]), 2)
        torch_fwd_bwd()
        want = [t.grad.clone() for t in (h_dst, h_src, att)]
        fwd_bwd()
        res["max_rel_diff_to_torch_gradients"] = max(
            float((t.grad - w).abs().max() / w.abs().max()) for t, w in zip((h_dst, h_src, att), want))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--heads", type=int, default=8)
    ap.add_argument("--features", default="8,16", help="columns per head, comma-separated")
    ap.add_argument("--no-torch", action="store_true", help="skip the torch formulation")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rowptr, col, val, n = graphgen.make_graph("reddit", device=dev, seed=1, scale=args.scale)
    nnz = int(col.numel())
    lens = (rowptr[1:] - rowptr[:-1]).long()
    adj = gcn_amd.CsrAdjacency(rowptr, col, val, (n, n), symmetric=True)
    T = lambda fn: time_ms(fn, args.steps, args.warmup)
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    res = {"graph": "reddit", "n": n, "nnz": nnz, "scale": args.scale, "steps": args.steps, "warmup": args.warmup,
           "rounds": args.rounds, "max_row": int(lens.max()), "mean_row": round(nnz / max(n, 1), 1),
           "what": "ms per call, CUDA events around `steps` calls after `warmup` calls; one figure per round", "shapes": []}
    for F in (int(f) for f in args.features.split(",")):
        res["shapes"].append(one_shape(adj, n, nnz, args.heads, F, T, args.rounds, gen, dev, not args.no_torch))
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

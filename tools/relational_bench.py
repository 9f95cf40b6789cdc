#!/usr/bin/env python3
"""Relation-typed aggregation (gcn_amd.relation_aggregate, gcn_amd/csrc/relational.hip) on the Reddit-shaped graph
(graphgen.make_graph("reddit")) with uniformly random edge types: milliseconds of the forward and of forward + backward
(gradients in x, coeff and V) of the message part of a basis R-GCN layer, [n, k] -> [n, k], at k in {64, 128}, B in
{2, 8} bases and R in {8, 64} relations, three ways:

  * new:    relation_aggregate(types, x, coeff, v) @ V.view(B k, k) — one gather per entry, B planes;
  * heads:  spmm_heads(adj, x @ V', w) with w[e, b] = coeff[etype[e], b] v[e], an [nnz, B] array, then the sum over the B
            heads — a B k wide row gathered per entry;
  * loop:   R spmm calls, one per relation's own adjacency (built outside the timed region), their [n, R k] results
            against the [R k, k] matrix of sum_b coeff[t, b] V[b].

Times are CUDA events around `steps` calls after `warmup` calls (fewer where one call takes so long that `steps` of them
would pass 1.5 s); the variants alternate inside each of `repeats` rounds, and every figure is reported as the median
with the lowest and highest round, so the spread is in the result.  The three outputs are checked against each other.
Prints one JSON line and writes it to --out (default: relational_bench.json in the profiles directory), which is
rewritten after every shape, so a run that is cut short leaves what it measured ("error_check": "incomplete").

    python tools/relational_bench.py [--steps 10] [--warmup 3] [--repeats 5] [--scale 1.0] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import gcn_amd                  # noqa: E402
from gcn_amd import graphgen    # noqa: E402


def time_ms(fn, steps, warmup, window_ms=1500.0):
    """ms per call; a call that takes long gets fewer steps (at least one) so that a window stays near `window_ms`"""
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    probe = (time.perf_counter() - t0) * 1e3
    steps = max(1, min(steps, int(window_ms / max(probe, 1e-3))))
    for _ in range(min(warmup, steps)):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def spread(samples):
    return {"median_ms": round(statistics.median(samples), 4), "min_ms": round(min(samples), 4), "max_ms": round(max(samples), 4)}


def relation_adjacencies(adj, etype, values, R):
    """one CsrAdjacency per relation: the entries of that type, weighted by values"""
    rp = adj.rowptr.long()
    rows = torch.repeat_interleave(torch.arange(adj.m, device=adj.device), rp[1:] - rp[:-1], output_size=adj.nnz)
    out = []
    for t in range(R):
        of = etype == t
        rowptr = torch.zeros(adj.m + 1, dtype=torch.int64, device=adj.device)
        rowptr[1:] = torch.cumsum(torch.bincount(rows[of], minlength=adj.m), 0)
        out.append(gcn_amd.CsrAdjacency(rowptr.to(torch.int32), adj.col[of], values[of], (adj.m, adj.n), symmetric=False))
    return out


def measure(adj, types, values, parts, k, B, R, steps, warmup, repeats):
    dev = adj.device
    gen = torch.Generator(device=dev)
    gen.manual_seed(1000 * k + 10 * B + R)
    x = torch.randn((adj.n, k), generator=gen, device=dev).requires_grad_(True)
    coeff = torch.randn((R, B), generator=gen, device=dev).requires_grad_(True)
    V = (torch.randn((B, k, k), generator=gen, device=dev) / k ** 0.5).requires_grad_(True)
    g = torch.randn((adj.m, k), generator=gen, device=dev)
    et = types.etype.long()

    def new():
        return gcn_amd.relation_aggregate(types, x, coeff, values) @ V.view(B * k, k)

    def heads():
        z = x @ V.permute(1, 0, 2).reshape(k, B * k)                   # [n, B k]: head b = x @ V[b]
        return gcn_amd.spmm_heads(adj, z, coeff[et] * values[:, None]).view(adj.m, B, k).sum(1)

    def loop():
        y = torch.cat([gcn_amd.spmm(a, x) for a in parts], 1)             # [m, R k]
        return y @ torch.einsum("tb,bio->tio", coeff, V).reshape(R * k, k)

    variants = {"new": new, "heads": heads, "loop": loop}
    with torch.no_grad():
        ref = new()
        scale = float(ref.abs().max())
        check = {name: round(float((fn() - ref).abs().max()) / scale, 8) for name, fn in variants.items() if name != "new"}
    ok = all(v <= 1e-4 for v in check.values())
    del ref
    samples = {name: ([], []) for name in variants}
    for _ in range(repeats):                               # the variants alternate: a drift of the machine hits all three
        for name, fn in variants.items():
            with torch.no_grad():
                samples[name][0].append(time_ms(fn, steps, warmup))
            samples[name][1].append(time_ms(lambda: torch.autograd.grad(fn(), (x, coeff, V), g), steps, warmup))
            print(f"# k={k} B={B} R={R} {name}: fwd {samples[name][0][-1]:.3f} ms, fwd_bwd {samples[name][1][-1]:.3f} ms", file=sys.stderr, flush=True)
    row = {"k": k, "B": B, "R": R, "relative_difference_to_new": check}
    for name, (f, fb) in samples.items():
        row[name] = {"fwd": spread(f), "fwd_bwd": spread(fb)}
    for what in ("fwd", "fwd_bwd"):
        for other in ("heads", "loop"):
            row[f"{other}_over_new_{what}"] = round(row[other][what]["median_ms"] / row["new"][what]["median_ms"], 3)
    print(f"# {row}", file=sys.stderr, flush=True)
    return row, ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("relational_bench: no GPU (there is no CPU path and nothing to time without one)", file=sys.stderr)
        return 2
    dev = torch.device("cuda:0")
    rowptr, col, val, n = graphgen.make_graph("reddit", device=dev, seed=1, scale=args.scale)
    adj = gcn_amd.CsrAdjacency(rowptr, col, val, (n, n), symmetric=True)
    res = {"graph": "reddit", "scale": args.scale, "n": n, "nnz": adj.nnz, "steps": args.steps, "warmup": args.warmup,
           "repeats": args.repeats, "device": torch.cuda.get_device_name(dev),
           "what": "ms per call of the message part of a basis R-GCN layer, [n, k] -> [n, k], CUDA events around `steps` calls "
                   "(fewer where `steps` calls would pass 1.5 s); "
                   "median, lowest and highest of `repeats` alternating rounds; fwd_bwd: gradients in x, coeff and V",
           "shapes": []}
    ok = True
    out = args.out or os.path.join(ROOT, "profiles", "relational_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)

    def write(status):                                     # after every shape: a run that is cut short leaves what it measured
        res["error_check"] = status
        with open(out, "w") as f:
            f.write(json.dumps(res) + "\n")

    for R in (8, 64):
        etype = torch.randint(0, R, (adj.nnz,), generator=torch.Generator(device=dev).manual_seed(R), device=dev, dtype=torch.int32)
        types = gcn_amd.EdgeTypes(adj, etype, R)
        values = types.norm()
        parts = relation_adjacencies(adj, etype, values, R)
        for k in (64, 128):
            for B in (2, 8):
                row, good = measure(adj, types, values, parts, k, B, R, args.steps, args.warmup, args.repeats)
                res["shapes"].append(row)
                ok = ok and good
                write("incomplete")
        del parts
    write("pass" if ok else "FAIL")
    print(json.dumps(res))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

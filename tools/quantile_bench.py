#!/usr/bin/env python3
"""Quantile / median aggregation (gcn_amd.aggregate_quantile, gcn_amd/csrc/aggregate_quantile.hip) on the Reddit-shaped
graph (graphgen.make_graph("reddit"): rows of hundreds of entries, the wave's radix select) and on a fanout-10 sampled
block of it (rows of at most 10 entries, the sorting network), at k = 64 and 128: milliseconds of

  * median:     aggregate_quantile(adj, x, 0.5), forward and forward + backward;
  * quartiles:  aggregate_quantile(adj, x, (0.25, 0.5, 0.75)), forward — three ranks off the same gathers;
  * one_max:    aggregate(adj, x, "max"), forward and forward + backward — one gather per entry, the floor a selection
                sits on;
  * padded_sort (the sampled block only): the median outside HIP — every neighbourhood padded to the longest row,
                x[index] of shape [m, d_max, k], torch.sort, one rank read off.  On the full graph that tensor is
                m * d_max * k elements and is not formed; the tool states its size instead.

Times are CUDA events around `steps` calls after `warmup` calls; the variants alternate inside each of `repeats` rounds, and
every figure is reported as the median with the lowest and highest round, so the spread is in the result.  The median is
checked against the padded sort on the block (equal values) and q = 1 against one_max on both graphs.  Prints one JSON line
and writes it to --out (default: quantile_bench.json in the profiles directory).

    python tools/quantile_bench.py [--steps 10] [--warmup 3] [--repeats 5] [--scale 1.0] [--seeds 65536] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import gcn_amd                  # noqa: E402
from gcn_amd import graphgen    # noqa: E402

QUARTILES = (0.25, 0.5, 0.75)


def time_ms(fn, steps, warmup):
    for _ in range(warmup):
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


def padded_sort(adj, k):
    """x -> the lower median by the padded formulation; the index tensor and the ranks are built once, outside the timing"""
    rp, lens = adj.rowptr.long(), (adj.rowptr[1:] - adj.rowptr[:-1]).long()
    dmax = int(lens.max())
    pos = torch.arange(dmax, device=adj.device)[None, :]
    at = (rp[:-1, None] + pos).clamp(max=adj.nnz - 1)
    index = torch.where(pos < lens[:, None], adj.col.long()[at], adj.n)       # row n of the padded table: +inf, sorts last
    rank = ((lens - 1).clamp(min=0).double() * 0.5).floor().long()
    rows = torch.arange(adj.m, device=adj.device)
    pad = torch.full((1, k), float("inf"), device=adj.device)
    empty = (lens == 0)[:, None]
    return lambda x: torch.cat([x, pad])[index].sort(dim=1).values[rows, rank].masked_fill(empty, 0.0)


def measure(adj, k, steps, warmup, repeats, with_padded):
    dev = adj.device
    gen = torch.Generator(device=dev)
    gen.manual_seed(k)
    x = torch.randn((adj.n, k), generator=gen, device=dev).requires_grad_(True)
    g = torch.randn((adj.m, k), generator=gen, device=dev)
    xd = x.detach()
    variants = {
        "median_fwd": lambda: gcn_amd.aggregate_quantile(adj, xd, 0.5),
        "one_max_fwd": lambda: gcn_amd.aggregate(adj, xd, "max"),
        "quartiles_fwd": lambda: gcn_amd.aggregate_quantile(adj, xd, QUARTILES),
        "median_fwd_bwd": lambda: torch.autograd.grad(gcn_amd.aggregate_quantile(adj, x, 0.5), x, g),
        "one_max_fwd_bwd": lambda: torch.autograd.grad(gcn_amd.aggregate(adj, x, "max"), x, g),
    }
    check = {"q1_equals_max": bool(torch.equal(gcn_amd.aggregate_quantile(adj, xd, 1.0), variants["one_max_fwd"]()))}
    if with_padded:
        padded = padded_sort(adj, k)
        variants["padded_sort_fwd"] = lambda: padded(xd)
        check["median_equals_padded_sort"] = bool(torch.equal(variants["median_fwd"](), padded(xd)))
    samples = {name: [] for name in variants}
    for _ in range(repeats):                               # the variants alternate: a drift of the machine hits all of them
        for name, fn in variants.items():
            samples[name].append(time_ms(fn, steps, warmup))
    row = {"k": k, "check": check}
    row.update({name: spread(s) for name, s in samples.items()})
    ratio = lambda a, b: {"of_medians": round(row[a]["median_ms"] / row[b]["median_ms"], 3),
                          "lowest": round(row[a]["min_ms"] / row[b]["max_ms"], 3), "highest": round(row[a]["max_ms"] / row[b]["min_ms"], 3)}
    row["median_over_one_max_fwd"] = ratio("median_fwd", "one_max_fwd")
    row["quartiles_over_median_fwd"] = ratio("quartiles_fwd", "median_fwd")
    row["median_over_one_max_fwd_bwd"] = ratio("median_fwd_bwd", "one_max_fwd_bwd")
    if with_padded:
        row["padded_sort_over_median_fwd"] = ratio("padded_sort_fwd", "median_fwd")
    print(f"# {row}", file=sys.stderr, flush=True)
    return row, all(check.values())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--seeds", type=int, default=65536)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("quantile_bench: no GPU (there is no CPU path and nothing to time without one)", file=sys.stderr)
        return 2
    dev = torch.device("cuda:0")
    rowptr, col, val, n = graphgen.make_graph("reddit", device=dev, seed=1, scale=args.scale)
    full = gcn_amd.CsrAdjacency(rowptr, col, val, (n, n), symmetric=True)
    seeds = torch.randperm(n, device=dev, generator=torch.Generator(device=dev).manual_seed(1))[:min(args.seeds, n)].int()
    (blk,), _ids = gcn_amd.sample_blocks(full, seeds, [10], seed=1)
    dmax = int((rowptr[1:] - rowptr[:-1]).max())
    res = {"graph": "reddit", "scale": args.scale, "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats,
           "device": torch.cuda.get_device_name(dev),
           "what": "ms per call, CUDA events around `steps` calls; median, lowest and highest of `repeats` alternating rounds; "
                   "a ratio is given of the medians, and as lowest / highest from the opposite extremes of the two spreads",
           "cases": []}
    ok = True
    for name, adj, with_padded in (("full", full, False), ("block_fanout10", blk.adj, True)):
        case = {"case": name, "m": adj.m, "n": adj.n, "nnz": adj.nnz, "widths": []}
        if not with_padded:
            case["padded_sort"] = (f"not formed: m * d_max * k = {adj.m} * {dmax} * 64 fp32 elements is "
                                   f"{adj.m * dmax * 64 * 4 / 2 ** 30:.0f} GiB at k = 64")
        for k in (64, 128):
            row, good = measure(adj, k, args.steps, args.warmup, args.repeats, with_padded)
            case["widths"].append(row)
            ok = ok and good
        res["cases"].append(case)
    res["error_check"] = "pass" if ok else "FAIL"
    line = json.dumps(res)
    print(line)
    out = args.out or os.path.join(ROOT, "profiles", "quantile_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

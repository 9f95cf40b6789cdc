#!/usr/bin/env python3
"""One-pass multi-aggregation (gcn_amd.aggregate_multi, gcn_amd/csrc/aggregate_multi.hip) on the Reddit-shaped graph
(graphgen.make_graph("reddit")) at k = 64 and 128: milliseconds of the forward and of forward + backward of

  * multi:   aggregate_multi(adj, x, ("mean", "max", "min", "std")) — one gather per entry;
  * pieces:  the same four planes from the units it replaces — aggregate max, min and mean, and the variance as
             aggregate(x * x, "mean") - aggregate(x, "mean") ** 2 (five walks; the cancellation-prone formula);
  * one_max: a single aggregate(adj, x, "max") — the same engine with one state per column.

Times are CUDA events around `steps` calls after `warmup` calls; the three variants alternate inside each of `repeats`
rounds, and every figure is reported as the median with the lowest and highest round, so the spread is in the result.
The planes of `multi` are checked against `pieces` (max / min equal; mean to the standing bound of the fp32 sums).  Prints
one JSON line and writes it to --out (default: aggregate_multi_bench.json in the profiles directory).

    python tools/aggregate_multi_bench.py [--steps 20] [--warmup 5] [--repeats 5] [--scale 1.0] [--out FILE]
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

REDUCE = ("mean", "max", "min", "std")
EPS = 1e-5


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


def pieces(adj, x):
    mean = gcn_amd.aggregate(adj, x, "mean")
    var = (gcn_amd.aggregate(adj, x * x, "mean") - mean * mean).clamp(min=0)
    return torch.cat([mean, gcn_amd.aggregate(adj, x, "max"), gcn_amd.aggregate(adj, x, "min"), (var + EPS).sqrt()], 1)


def spread(samples):
    return {"median_ms": round(statistics.median(samples), 4), "min_ms": round(min(samples), 4), "max_ms": round(max(samples), 4)}


def measure(adj, k, steps, warmup, repeats):
    dev = adj.device
    gen = torch.Generator(device=dev)
    gen.manual_seed(k)
    x = torch.randn((adj.n, k), generator=gen, device=dev).requires_grad_(True)
    g4 = torch.randn((adj.m, 4 * k), generator=gen, device=dev)
    g1 = g4[:, :k].contiguous()
    xd = x.detach()
    variants = {
        "multi": (lambda: gcn_amd.aggregate_multi(adj, xd, REDUCE, EPS),
                  lambda: torch.autograd.grad(gcn_amd.aggregate_multi(adj, x, REDUCE, EPS), x, g4)),
        "pieces": (lambda: pieces(adj, xd), lambda: torch.autograd.grad(pieces(adj, x), x, g4)),
        "one_max": (lambda: gcn_amd.aggregate(adj, xd, "max"), lambda: torch.autograd.grad(gcn_amd.aggregate(adj, x, "max"), x, g1)),
    }
    got, ref = variants["multi"][0](), variants["pieces"][0]()
    mag = gcn_amd.aggregate(adj, xd.abs(), "mean")
    check = {"max_min_equal": bool(torch.equal(got[:, k:3 * k], ref[:, k:3 * k])),
             "mean_error_over_bound": round(float(((got[:, :k] - ref[:, :k]).abs() / (2e-5 * mag + 1e-30)).max()), 4)}
    ok = check["max_min_equal"] and check["mean_error_over_bound"] <= 1.0
    del got, ref, mag
    samples = {name: ([], []) for name in variants}
    for _ in range(repeats):                               # the variants alternate: a drift of the machine hits all three
        for name, (fwd, fwd_bwd) in variants.items():
            samples[name][0].append(time_ms(fwd, steps, warmup))
            samples[name][1].append(time_ms(fwd_bwd, steps, warmup))
    row = {"k": k, "check": check}
    for name, (f, fb) in samples.items():
        row[name] = {"fwd": spread(f), "fwd_bwd": spread(fb)}
    for what in ("fwd", "fwd_bwd"):
        row[f"pieces_over_multi_{what}"] = round(row["pieces"][what]["median_ms"] / row["multi"][what]["median_ms"], 3)
        row[f"multi_over_one_max_{what}"] = round(row["multi"][what]["median_ms"] / row["one_max"][what]["median_ms"], 3)
    print(f"# {row}", file=sys.stderr, flush=True)
    return row, ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("aggregate_multi_bench: no GPU (there is no CPU path and nothing to time without one)", file=sys.stderr)
        return 2
    dev = torch.device("cuda:0")
    rowptr, col, val, n = graphgen.make_graph("reddit", device=dev, seed=1, scale=args.scale)
    adj = gcn_amd.CsrAdjacency(rowptr, col, val, (n, n), symmetric=True)
    res = {"graph": "reddit", "scale": args.scale, "n": n, "nnz": adj.nnz, "steps": args.steps, "warmup": args.warmup,
           "repeats": args.repeats, "reduce": list(REDUCE), "device": torch.cuda.get_device_name(dev),
           "what": "ms per call, CUDA events around `steps` calls; median, lowest and highest of `repeats` alternating rounds",
           "widths": []}
    ok = True
    for k in (64, 128):
        row, good = measure(adj, k, args.steps, args.warmup, args.repeats)
        res["widths"].append(row)
        ok = ok and good
    res["error_check"] = "pass" if ok else "FAIL"
    line = json.dumps(res)
    print(line)
    out = args.out or os.path.join(ROOT, "profiles", "aggregate_multi_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

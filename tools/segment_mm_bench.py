#!/usr/bin/env python3
"""The grouped matrix product (gcn_amd.segment_matmul, gcn_amd/csrc/segment_mm.hip) and the grouped RGCNConv, in milliseconds.

  * segment_matmul(x, segptr, W), [N, k] -> [N, k] at N = 2^20 and k = 64, against a Python loop of torch.mm per segment
    (rocBLAS, one launch per segment), at T in {8, 64, 512} segments of equal lengths and of skewed ones (lengths
    proportional to 1 / (t + 1), so the first segment holds a large share and the last ones a few rows); forward, and forward +
    backward (gradients in x and W).
  * RGCNConv(k, k, R, grouped=True) on the Reddit-shaped graph (graphgen.make_graph("reddit"), --scale 0.25 by default: the
    workload of tools/relational_bench.py at a quarter) with uniformly random types, forward and forward + backward, at
    R = 8 against the typed-mode layer RGCNConv(k, k, R) loaded from the same state_dict, and alone at R in {64, 512}: the
    typed mode is not run there (its [m, R k] planes, reported per row as typed_planes_GiB, and its R / 8 gather passes are
    what the grouped path exists to avoid).

Times are CUDA events around `steps` calls after `warmup` calls (fewer where `steps` calls would pass 1.5 s); the variants
alternate inside each of `repeats` rounds and every figure is the median with the lowest and highest round.  Outputs of the
variants are checked against each other.  Prints one JSON line and writes it to --out (default: segment_mm_bench.json in the
profiles directory), rewritten after every shape ("error_check": "incomplete" until the end).

    python tools/segment_mm_bench.py [--steps 10] [--warmup 3] [--repeats 5] [--scale 0.25] [--out FILE]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gcn_amd                                  # noqa: E402
from gcn_amd import graphgen                    # noqa: E402
from relational_bench import spread, time_ms    # noqa: E402


def rounds(variants, grads, g, steps, warmup, repeats, tag):
    """{name: {"fwd": spread, "fwd_bwd": spread}}; the variants alternate inside every round"""
    samples = {name: ([], []) for name in variants}
    for _ in range(repeats):
        for name, fn in variants.items():
            with torch.no_grad():
                samples[name][0].append(time_ms(fn, steps, warmup))
            samples[name][1].append(time_ms(lambda: torch.autograd.grad(fn(), grads[name], g), steps, warmup))
            print(f"# {tag} {name}: fwd {samples[name][0][-1]:.3f} ms, fwd_bwd {samples[name][1][-1]:.3f} ms", file=sys.stderr, flush=True)
    return {name: {"fwd": spread(f), "fwd_bwd": spread(fb)} for name, (f, fb) in samples.items()}


def measure_matmul(dev, N, k, T, skewed, steps, warmup, repeats):
    gen = torch.Generator(device=dev).manual_seed(T + skewed)
    share = 1.0 / torch.arange(1, T + 1, dtype=torch.float64) if skewed else torch.ones(T, dtype=torch.float64)
    lens = torch.floor(share / share.sum() * N).long()
    lens[0] += N - int(lens.sum())
    bounds = [0] + torch.cumsum(lens, 0).tolist()
    segptr = torch.tensor(bounds, dtype=torch.int32, device=dev)
    x = torch.randn((N, k), generator=gen, device=dev).requires_grad_(True)
    W = (torch.randn((T, k, k), generator=gen, device=dev) / k ** 0.5).requires_grad_(True)
    g = torch.randn((N, k), generator=gen, device=dev)
    variants = {"segment_matmul": lambda: gcn_amd.segment_matmul(x, segptr, W),
                "mm_loop": lambda: torch.cat([torch.mm(x[bounds[t]:bounds[t + 1]], W[t]) for t in range(T)], 0)}
    with torch.no_grad():
        ref = variants["mm_loop"]()
        diff = float((variants["segment_matmul"]() - ref).abs().max() / ref.abs().max())
    row = {"N": N, "k": k, "T": T, "lengths": "skewed" if skewed else "equal", "longest": int(lens.max()), "shortest": int(lens.min()),
           "relative_difference": round(diff, 8)}
    row.update(rounds(variants, {name: (x, W) for name in variants}, g, steps, warmup, repeats, f"T={T} {row['lengths']}"))
    for what in ("fwd", "fwd_bwd"):
        row[f"mm_loop_over_segment_matmul_{what}"] = round(row["mm_loop"][what]["median_ms"] / row["segment_matmul"][what]["median_ms"], 3)
    return row, diff <= 1e-4


def measure_layer(adj, k, R, steps, warmup, repeats):
    dev = adj.device
    etype = torch.randint(0, R, (adj.nnz,), generator=torch.Generator(device=dev).manual_seed(R), device=dev, dtype=torch.int32)
    types = gcn_amd.EdgeTypes(adj, etype, R)
    values = types.norm()
    torch.manual_seed(R)
    layers = {"grouped": gcn_amd.RGCNConv(k, k, R, grouped=True).to(dev)}
    row = {"k": k, "R": R, "typed_planes_GiB": round(adj.m * R * k * 4 / 2 ** 30, 2)}
    if R <= 8:
        layers["typed"] = gcn_amd.RGCNConv(k, k, R).to(dev)
        layers["typed"].load_state_dict(layers["grouped"].state_dict())
    else:
        row["typed"] = "not run: infeasible at this R (the [m, R k] planes, R / 8 gather passes)"
    gen = torch.Generator(device=dev).manual_seed(R + 1)
    x = torch.randn((adj.n, k), generator=gen, device=dev).requires_grad_(True)
    g = torch.randn((adj.m, k), generator=gen, device=dev)
    variants = {name: (lambda layer=layer: layer(types, x, values)) for name, layer in layers.items()}
    diff = 0.0
    if "typed" in variants:
        with torch.no_grad():
            ref = variants["typed"]()
            diff = float((variants["grouped"]() - ref).abs().max() / ref.abs().max())
        row["relative_difference"] = round(diff, 8)
    row.update(rounds(variants, {name: (x, *layer.parameters()) for name, layer in layers.items()}, g, steps, warmup, repeats, f"RGCNConv R={R}"))
    if "typed" in variants:
        for what in ("fwd", "fwd_bwd"):
            row[f"typed_over_grouped_{what}"] = round(row["typed"][what]["median_ms"] / row["grouped"][what]["median_ms"], 3)
    return row, diff <= 1e-4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--scale", type=float, default=0.25)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("segment_mm_bench: no GPU (there is no CPU path and nothing to time without one)", file=sys.stderr)
        return 2
    dev = torch.device("cuda:0")
    rowptr, col, val, n = graphgen.make_graph("reddit", device=dev, seed=1, scale=args.scale)
    adj = gcn_amd.CsrAdjacency(rowptr, col, val, (n, n), symmetric=True)
    res = {"graph": "reddit", "scale": args.scale, "n": n, "nnz": adj.nnz, "steps": args.steps, "warmup": args.warmup,
           "repeats": args.repeats, "device": torch.cuda.get_device_name(dev),
           "what": "ms per call, CUDA events around `steps` calls (fewer where `steps` calls would pass 1.5 s); median, lowest and "
                   "highest of `repeats` alternating rounds; fwd_bwd: gradients in x and every weight",
           "segment_matmul": [], "rgcn_conv": []}
    out = args.out or os.path.join(ROOT, "profiles", "segment_mm_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    ok = True

    def add(key, result):
        nonlocal ok
        row, good = result
        res[key].append(row)
        ok = ok and good
        res["error_check"] = "incomplete"
        print(f"# {row}", file=sys.stderr, flush=True)
        with open(out, "w") as f:
            f.write(json.dumps(res) + "\n")

    for T in (8, 64, 512):
        for skewed in (False, True):
            add("segment_matmul", measure_matmul(dev, 1 << 20, 64, T, skewed, args.steps, args.warmup, args.repeats))
    for R in (8, 64, 512):
        add("rgcn_conv", measure_layer(adj, 64, R, args.steps, args.warmup, args.repeats))
    res["error_check"] = "pass" if ok else "FAIL"
    with open(out, "w") as f:
        f.write(json.dumps(res) + "\n")
    print(json.dumps(res))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

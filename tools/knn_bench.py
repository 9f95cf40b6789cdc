#!/usr/bin/env python3
"""The device k-nearest-neighbour search (gcn_amd/knn.py, gcn_amd/csrc/knn.hip) against the torch formulation on the same
device — torch.cdist + topk, chunked over the queries so that a chunk's distance matrix stays below 1 GiB — on three shapes:
  point_cloud      n = 100 000 points, d = 3, k = 16, every point a query (self excluded)
  hgnn_features    n = 12 311 vertices, d = 6 144, k = 10 (the reference HGNN's feature matrix; self excluded)
  few_queries      q = 1 024 queries against n = 1 000 000 candidates, d = 64, k = 32
Per shape, ms per call of both sides, timed with device events around `steps` calls, `steps` chosen so that a window lasts
about 0.2 s (at least one call).  The two sides alternate, `--rounds` windows each: the median is reported, and the spread is
(max - min) / median of a side's windows.  `agreement` is the share of torch's neighbours that gcn_amd.knn returns too (torch
computes |x|^2 + |y|^2 - 2 x.y for these sizes, so the last places of a distance, and with them a neighbour at the k-th place,
may differ; gcn_amd's own result is checked exactly by the tests).
The model: flops = 3 q n d (a subtraction and a fused multiply-add per pair and column); compulsory bytes =
4 d (q + n) + 8 q k; staged bytes = what the workgroups load, 4 d (ceil(q / 64) n + ceil(n / 64) q), plus the part keys.
Prints one JSON line and writes it to the profiles directory as knn_bench.json (--out FILE: elsewhere).

    python tools/knn_bench.py [--rounds 5] [--scale 1.0] [--out FILE]
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

import gcn_amd                                  # noqa: E402
from gcn_amd import _lib                        # noqa: E402


def torch_knn(x, y, k, exclude_self):
    chunk = max(1, (1 << 28) // max(int(y.shape[0]), 1))
    out = []
    for r0 in range(0, x.shape[0], chunk):
        dist = torch.cdist(x[r0:r0 + chunk], y)
        if exclude_self:
            rows = torch.arange(r0, min(r0 + chunk, x.shape[0]), device=x.device)
            dist[rows - r0, rows] = float("inf")
        out.append(dist.topk(k, dim=1, largest=False).indices)
    return torch.cat(out)


def window_ms(fn, steps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(steps):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / steps


def compare(new, old, rounds):
    res = {}
    steps = {}
    for name, fn in (("new", new), ("old", old)):
        fn()                                               # warm-up: code objects, allocator, library heuristics
        once = window_ms(fn, 1)
        steps[name] = max(1, min(200, int(200.0 / max(once, 1e-3))))
    times = {"new": [], "old": []}
    for _ in range(rounds):
        for name, fn in (("new", new), ("old", old)):
            times[name].append(window_ms(fn, steps[name]))
    for name in ("new", "old"):
        med = statistics.median(times[name])
        res[name + "_ms"] = round(med, 4)
        res[name + "_spread"] = round((max(times[name]) - min(times[name])) / med, 3)
        res[name + "_steps"] = steps[name]
    res["old_over_new"] = round(res["old_ms"] / res["new_ms"], 3)
    return res


def measure(name, x, y, k, exclude_self, rounds):
    q, d, n = int(x.shape[0]), int(x.shape[1]), int(y.shape[0])
    idx, _ = gcn_amd.knn(x, k, y=None if y is x else y, exclude_self=exclude_self)
    ref = torch_knn(x, y, k, exclude_self)
    both = (idx.long().unsqueeze(2) == ref.unsqueeze(1)).any(dim=1) if q * k * k <= (1 << 28) else None
    if both is None:                                       # (row chunks: q k^2 comparisons)
        hits = 0
        for r0 in range(0, q, 8192):
            hits += int((idx[r0:r0 + 8192].long().unsqueeze(2) == ref[r0:r0 + 8192].unsqueeze(1)).any(dim=1).sum())
    else:
        hits = int(both.sum())
    splits = int(_lib.load().gcn_knn_splits(q, n, 0))
    qb, tiles = -(-q // _lib.KNN_TILE_Q), -(-n // _lib.KNN_TILE_C)
    row = {"shape": name, "q": q, "n": n, "d": d, "k": k, "exclude_self": exclude_self, "splits": splits,
           "agreement": round(hits / (q * k), 6)}
    row["knn"] = compare(lambda: gcn_amd.knn(x, k, y=None if y is x else y, exclude_self=exclude_self),
                         lambda: torch_knn(x, y, k, exclude_self), rounds)
    row["model_flops"] = 3 * q * n * d
    row["model_bytes_compulsory"] = 4 * d * (q + n) + 8 * q * k
    row["model_bytes_staged"] = 4 * d * (qb * n + tiles * q) + 2 * 8 * q * splits * k + 8 * q * k
    sec = row["knn"]["new_ms"] * 1e-3
    row["model_tflops"] = round(row["model_flops"] / sec / 1e12, 3)
    row["model_staged_gb_per_s"] = round(row["model_bytes_staged"] / sec / 1e9, 1)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device="cpu")
    res = {"rounds": args.rounds, "scale": args.scale, "device": torch.cuda.get_device_name(dev),
           "what": "ms per call, median of `rounds` alternating windows of about 0.2 s timed with device events; new = gcn_amd.knn, "
                   "old = torch.cdist + topk chunked over queries; spread = (max - min) / median",
           "shapes": []}

    def points(rows, d, seed):
        gen.manual_seed(seed)
        return torch.randn((max(64, int(rows * args.scale)), d), generator=gen).to(dev)

    def run(name, x, y, k, exclude_self):
        row = measure(name, x, y, k, exclude_self, args.rounds)
        res["shapes"].append(row)
        print(f"# {row}", file=sys.stderr, flush=True)
        torch.cuda.empty_cache()

    x = points(100000, 3, 1)
    run("point_cloud", x, x, 16, True)
    x = points(12311, 6144, 2)
    run("hgnn_features", x, x, 10, True)
    del x
    run("few_queries", points(1024, 64, 3), points(1000000, 64, 4), 32, False)
    line = json.dumps(res)
    print(line)
    out = args.out or os.path.join(ROOT, "profiles", "knn_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

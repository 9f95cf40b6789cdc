#!/usr/bin/env python3
"""Farthest point sampling and segmented kNN (gcn_amd/points.py, gcn_amd/csrc/fps.hip, knn.hip) against what a user writes
without them, on PointNet++-like batches: 32 clouds of 1 024 / 4 096 / 16 384 points, d = 3.
  fps       gcn_amd.fps(x, ptr, ratio=0.25)  against the torch formulation batched over the clouds: per pick one distance
            update from differences (no cdist), one minimum and one argmax — a handful of launches per pick.
  knn       gcn_amd.knn(x, k, exclude_self=True, ptr_x=ptr), k = 16 and 32, against a Python loop of gcn_amd.knn over the
            clouds.
Per row, ms per call of both sides, timed with device events around `steps` calls, `steps` chosen so that a window lasts about
0.2 s (at least one call).  The two sides alternate, `--rounds` windows each: the median is reported, and the spread is
(max - min) / median of a side's windows.  `same` says whether the two sides returned the same picks / neighbours on these
float points (the torch side sums the squares in another order, so a pick may differ where two distances nearly tie; the
kernels' own results are checked exactly by the tests).
Prints one JSON line and writes it to the profiles directory as fps_bench.json (--out FILE: elsewhere).

    python tools/fps_bench.py [--rounds 5] [--clouds 32] [--out FILE]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import gcn_amd                                  # noqa: E402
from knn_bench import compare                   # noqa: E402  (alternating windows, device events)


def torch_fps(x, m):
    """x: [B, N, d] -> [B, m] local picks, every cloud from its row 0"""
    b, n, _ = x.shape
    dmin = torch.full((b, n), float("inf"), device=x.device)
    pick = torch.zeros(b, dtype=torch.long, device=x.device)
    rows = torch.arange(b, device=x.device)
    out = torch.empty((b, m), dtype=torch.long, device=x.device)
    for t in range(m):
        out[:, t] = pick
        d2 = (x - x[rows, pick].unsqueeze(1)).square().sum(dim=2)
        dmin = torch.minimum(dmin, d2)
        dmin[rows, pick] = -1.0
        pick = dmin.argmax(dim=1)
    return out


def looped_knn(x, ptr, k):
    out = []
    for lo, hi in zip(ptr, ptr[1:]):
        out.append(gcn_amd.knn(x[lo:hi], k, exclude_self=True)[0] + lo)
    return torch.cat(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--clouds", type=int, default=32)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device="cpu")
    res = {"rounds": args.rounds, "clouds": args.clouds, "device": torch.cuda.get_device_name(dev),
           "resident_points_d3": int(gcn_amd.load_library().gcn_fps_resident_points(3)),
           "what": "ms per call, median of `rounds` alternating windows of about 0.2 s timed with device events; fps: new = "
                   "gcn_amd.fps, old = torch per-pick update + argmax batched over the clouds; knn: new = gcn_amd.knn with ptr_x, "
                   "old = a Python loop of gcn_amd.knn over the clouds; spread = (max - min) / median",
           "rows": []}
    for points in (1024, 4096, 16384):
        gen.manual_seed(points)
        x = torch.randn((args.clouds * points, 3), generator=gen).to(dev)
        ptr = [b * points for b in range(args.clouds + 1)]
        m = points // 4
        idx, out_ptr = gcn_amd.fps(x, ptr, ratio=0.25)
        ref = torch_fps(x.view(args.clouds, points, 3), m) + torch.tensor(ptr[:-1], device=dev).unsqueeze(1)
        row = {"op": "fps", "clouds": args.clouds, "points": points, "picks": m, "same": bool(torch.equal(idx.long(), ref.reshape(-1)))}
        row.update(compare(lambda: gcn_amd.fps(x, ptr, ratio=0.25), lambda: torch_fps(x.view(args.clouds, points, 3), m), args.rounds))
        row["new_us_per_pick"] = round(row["new_ms"] * 1e3 / m, 3)
        res["rows"].append(row)
        print(f"# {row}", file=sys.stderr, flush=True)
        for k in (16, 32):
            seg = gcn_amd.knn(x, k, exclude_self=True, ptr_x=ptr)[0]
            row = {"op": "knn", "clouds": args.clouds, "points": points, "k": k, "same": bool(torch.equal(seg, looped_knn(x, ptr, k)))}
            row.update(compare(lambda: gcn_amd.knn(x, k, exclude_self=True, ptr_x=ptr), lambda: looped_knn(x, ptr, k), args.rounds))
            res["rows"].append(row)
            print(f"# {row}", file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    out = args.out or os.path.join(ROOT, "profiles", "fps_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Device CSR construction (gcn_amd/construct.py, gcn_amd/csrc/construct.hip) against what it replaces, on four shapes: a
sampled block (1 024 seeds, fanout 10) and a 50 000-seed block of the Reddit-shaped graph (bipartite, mostly buckets of one
or two entries), the Reddit-shaped graph itself (graphgen.make_graph("reddit"), 114.8 M entries, buckets of hundreds) and an
R-MAT whose hub column is far longer than the LDS tier holds.  Per shape, ms per call:
  pattern     CsrAdjacency._transposed_pattern()            vs  the torch formulation it replaced (tests/construct_ref.py)
  transpose   gcn_amd.transpose_csr (arrays + CsrAdjacency) vs  CSR -> COO -> .t().coalesce() -> CSR
  from_edges  gcn_amd.csr_from_edges on the shuffled edges  vs  torch.sparse_coo_tensor(...).coalesce().to_sparse_csr()
  bucket      the tiered bucketing of the columns alone     vs  one global stable pair sort: torch.sort(stable=True) on the
              int32 keys, which is one hipCUB DeviceRadixSort::SortPairs over (key, index), plus bincount and cumsum
Every time is a host clock around `steps` calls that end in a device synchronise (the torch formulations synchronise inside
anyway), `steps` chosen so that a window lasts about 0.2 s.  The two sides of a comparison alternate, `--rounds` windows
each: the median is reported, and the spread is (max - min) / median of a side's windows.  `slower_beyond_spread` marks a
comparison where the new median exceeds the old one by more than the larger of the two spreads.  Results are checked equal
first (bit for bit where the matrix has no repeated entries).
Prints one JSON line and writes it to the profiles directory as construct_bench.json (--out FILE: elsewhere).

    python tools/construct_bench.py [--rounds 5] [--scale 1.0] [--rmat-scale 21] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import gcn_amd                  # noqa: E402
from gcn_amd import _lib, construct, graphgen    # noqa: E402
from construct_ref import torch_coo_transpose, torch_transposed_pattern    # noqa: E402


def window_ms(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def compare(new, old, rounds):
    """alternating windows of the two sides -> dict of medians, spreads and the verdict"""
    new(); old()                                           # warm-up: code objects, the allocator's blocks, hipCUB's choices
    new(); old()
    steps = {}
    for name, fn in (("new", new), ("old", old)):
        steps[name] = max(1, min(200, int(0.2 / max(window_ms(fn, 1) * 1e-3, 1e-6))))
    t = {"new": [], "old": []}
    for _ in range(rounds):
        t["new"].append(window_ms(new, steps["new"]))
        t["old"].append(window_ms(old, steps["old"]))
    med = {k: statistics.median(v) for k, v in t.items()}
    spread = {k: (max(v) - min(v)) / med[k] for k, v in t.items()}
    return {"new_ms": round(med["new"], 4), "old_ms": round(med["old"], 4), "new_spread": round(spread["new"], 3),
            "old_spread": round(spread["old"], 3), "steps_per_window": steps, "old_over_new": round(med["old"] / med["new"], 2),
            "slower_beyond_spread": bool(med["new"] > med["old"] * (1 + max(spread.values())))}


def global_pair_sort(keys32, nbuckets):
    """the third contender: offsets and the stable permutation from one global radix sort of (key, index) pairs"""
    perm = torch.sort(keys32, stable=True).indices
    offsets = torch.zeros(nbuckets + 1, dtype=torch.int64, device=keys32.device)
    offsets[1:] = torch.cumsum(torch.bincount(keys32, minlength=nbuckets), 0)
    return offsets.to(torch.int32), perm.to(torch.int32)


def measure(name, adj, rounds, duplicate_free):
    dev = adj.device
    counts = adj.transpose().rowptr
    lens = (counts[1:] - counts[:-1]).long()
    row = {"shape": name, "m": adj.m, "n": adj.n, "nnz": adj.nnz, "longest_bucket": int(lens.max()),
           "buckets_of_0_or_1": int((lens < 2).sum()), "buckets_wave_tier": int(((lens >= 2) & (lens <= _lib.BUCKET_WAVE_MAX)).sum()),
           "buckets_block_tier": int(((lens > _lib.BUCKET_WAVE_MAX) & (lens <= _lib.BUCKET_BLOCK_MAX)).sum()),
           "buckets_long_tier": int((lens > _lib.BUCKET_BLOCK_MAX).sum())}
    # ---- equal results first ---------------------------------------------------------------------------------------------
    ok = all(a.dtype == b.dtype and bool(torch.equal(a, b)) for a, b in zip(adj._transposed_pattern(), torch_transposed_pattern(adj)))
    t, eid = gcn_amd.transpose_csr(adj)
    if duplicate_free:
        orp, oci, ova = torch_coo_transpose(adj)
        ok = ok and bool(torch.equal(t.rowptr, orp.to(torch.int32))) and bool(torch.equal(t.col, oci.to(torch.int32)))
        ok = ok and bool(torch.equal(t.val.view(torch.int32), ova.view(torch.int32)))
        del orp, oci, ova
    off_t, perm_t = construct._bucket(adj.col, adj.n)
    off_g, perm_g = global_pair_sort(adj.col, adj.n)
    ok = ok and bool(torch.equal(off_t, off_g)) and bool(torch.equal(perm_t, perm_g)) and bool(torch.equal(perm_t, eid))
    del t, eid, off_t, perm_t, off_g, perm_g
    gen = torch.Generator(device="cpu")
    gen.manual_seed(3)
    rp = adj.rowptr.long()
    rows = torch.repeat_interleave(torch.arange(adj.m, device=dev), rp[1:] - rp[:-1], output_size=adj.nnz)
    shuffle = torch.randperm(adj.nnz, generator=gen).to(dev)
    er, ec, ev = rows[shuffle], adj.col.long()[shuffle], adj.val[shuffle]
    del rows, shuffle, rp
    built, _ = gcn_amd.csr_from_edges(er, ec, (adj.m, adj.n), ev)
    ok = ok and bool(torch.equal(built.rowptr, adj.rowptr)) and bool(torch.equal(built.col, adj.col))
    if duplicate_free:
        ok = ok and bool(torch.equal(built.val, adj.val))
    del built
    row["equal"] = ok
    # ---- times -----------------------------------------------------------------------------------------------------------
    row["pattern"] = compare(lambda: adj._transposed_pattern(), lambda: torch_transposed_pattern(adj), rounds)
    row["transpose"] = compare(lambda: gcn_amd.transpose_csr(adj), lambda: torch_coo_transpose(adj), rounds)
    row["from_edges"] = compare(lambda: gcn_amd.csr_from_edges(er, ec, (adj.m, adj.n), ev),
                                lambda: torch.sparse_coo_tensor(torch.stack([er, ec]), ev, (adj.m, adj.n)).coalesce().to_sparse_csr(),
                                rounds)
    row["bucket"] = compare(lambda: construct._bucket(adj.col, adj.n), lambda: global_pair_sort(adj.col, adj.n), rounds)
    # the least traffic of a transpose: the keys twice (count, scatter), perm written, sorted in place (read + write), read by
    # the gather with the values, the three outputs; the cursor and offsets words per bucket
    least = adj.nnz * 4 * (2 + 1 + 2 + 2 + 2) + adj.n * 4 * 4
    row["transpose_least_bytes"] = least
    row["transpose_gb_per_s"] = round(least / (row["transpose"]["new_ms"] * 1e-3) / 1e9, 1)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--rmat-scale", type=int, default=21)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"rounds": args.rounds, "scale": args.scale, "wave_max": _lib.BUCKET_WAVE_MAX, "block_max": _lib.BUCKET_BLOCK_MAX,
           "what": "ms per call, median of `rounds` alternating windows of about 0.2 s (host clock, device synchronised); "
                   "new = the device kernels, old = the torch formulation named in the tool's header; bucket: new = tiered "
                   "bucketing, old = one global stable pair sort (hipCUB through torch.sort); spread = (max - min) / median",
           "shapes": []}
    rowptr, col, val, n = graphgen.make_graph("reddit", device=dev, seed=1, scale=args.scale)
    reddit = gcn_amd.CsrAdjacency(rowptr, col, val, (n, n), symmetric=False)
    gen = torch.Generator(device="cpu")
    gen.manual_seed(0)
    order = torch.randperm(n, generator=gen).to(dev)
    shapes = []
    for label, seeds in (("block_1024_seeds_fanout_10", 1024), ("block_50000_seeds_fanout_10", 50000)):
        blocks, _ = gcn_amd.sample_blocks(reddit, order[:min(seeds, n)], [10], seed=1, offset=0)
        b = blocks[0].adj
        shapes.append((label, gcn_amd.CsrAdjacency(b.rowptr, b.col, b.val, (b.m, b.n), symmetric=False), True))
    shapes.append(("reddit", reddit, True))
    ok = True
    for label, adj, dup_free in shapes:
        row = measure(label, adj, args.rounds, dup_free)
        ok = ok and row["equal"]
        res["shapes"].append(row)
        print(f"# {row}", file=sys.stderr, flush=True)
    del shapes, reddit, adj, rowptr, col, val
    torch.cuda.empty_cache()
    rowptr, col, val, n = graphgen.make_rmat(args.rmat_scale, device=dev)
    rmat = gcn_amd.CsrAdjacency(rowptr, col, val, (n, n), symmetric=False)
    row = measure(f"rmat_scale_{args.rmat_scale}", rmat, args.rounds, True)
    ok = ok and row["equal"]
    res["shapes"].append(row)
    print(f"# {row}", file=sys.stderr, flush=True)
    res["error_check"] = "pass" if ok else "FAIL"
    line = json.dumps(res)
    print(line)
    out = args.out or os.path.join(ROOT, "profiles", "construct_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

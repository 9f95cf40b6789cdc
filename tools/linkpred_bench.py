#!/usr/bin/env python3
"""Link prediction (gcn_amd.find_edges / negative_sample / LinkNeighborLoader, gcn_amd/csrc/lookup.hip) on the headline
graph (Reddit-shaped, graphgen.make_graph("reddit")), each against the torch formulation on the same GPU:

  find_edges over every stored entry          against 64-bit keys row * n + col and torch.searchsorted on the (ascending) key
                                              array of the pattern; the key array is built once, outside the timed window
  find_edges over 2^24 stored entries drawn   against the same (consecutive lanes no longer search the same row)
  at random
  negative_sample, 2^20 query rows x 1        against torch.randint, the same keys and searchsorted, and a resample loop
                                              that redraws the colliding slots until none collides (a host read per round)
  one LinkNeighborLoader batch (1024 entries, against the same batch with the torch negatives in the kernel's place
  one negative each, fanouts [10, 5])

Times are wall clock around work that ends in a device synchronise, ms per call; the two sides alternate in rounds and the
table gives each side's median and its spread (max - min over the rounds).  The lookup's results must be equal integer for
integer; the negatives come from different generators, so both sides are checked for what they promise: no drawn column is
stored in its row.  The kernels are latency-bound (a chain of dependent 4-byte probes per query): no bandwidth figure is
derived.  Prints one JSON line and writes it to the profiles directory as linkpred_bench.json (--out FILE: elsewhere).

    python tools/linkpred_bench.py [--steps 20] [--warmup 5] [--rounds 5] [--scale 1.0] [--out FILE]
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
from gcn_amd.coalesce import _entry_rows    # noqa: E402


def wall_ms(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def alternate(ours, theirs, steps, warmup, rounds):
    """→ {ours_ms, ours_spread_ms, torch_ms, torch_spread_ms, torch_over_ours}: the sides alternate, round by round"""
    a, b = [], []
    for _ in range(rounds):
        a.append(wall_ms(ours, steps, warmup))
        b.append(wall_ms(theirs, steps, warmup))
    ma, mb = statistics.median(a), statistics.median(b)
    return {"ours_ms": round(ma, 4), "ours_spread_ms": round(max(a) - min(a), 4), "torch_ms": round(mb, 4),
            "torch_spread_ms": round(max(b) - min(b), 4), "torch_over_ours": round(mb / ma, 2)}


def torch_find(keys, n, rows, cols):
    """the lookup in torch ops: the position of row * n + col in the ascending key array, -1 when it is not there"""
    q = rows.long() * n + cols.long()
    at = torch.searchsorted(keys, q).clamp(max=keys.numel() - 1)
    return torch.where(keys[at] == q, at, -1).to(torch.int32)


def torch_negatives(keys, n, rows, gen):
    """one negative per row: randint, keys, searchsorted, and a resample loop until no slot collides"""
    r = rows.long()
    out = torch.randint(0, n, r.shape, device=r.device, generator=gen)
    bad = torch.nonzero((torch_find(keys, n, r, out) >= 0) | (out == r)).squeeze(1)
    while bad.numel():                                     # (numel: the host read of every round)
        out[bad] = torch.randint(0, n, bad.shape, device=r.device, generator=gen)
        bad = bad[(torch_find(keys, n, r[bad], out[bad]) >= 0) | (out[bad] == r[bad])]
    return out


def torch_batch(adj, keys, e, fanouts, gen, seed, offset):
    """one loader batch with torch_negatives in the place of the kernel (the same remaining ops)"""
    rows = torch.searchsorted(adj.rowptr.long(), e, right=True) - 1
    u = torch.cat([rows, rows])
    v = torch.cat([adj.col[e].long(), torch_negatives(keys, adj.n, rows, gen)])
    nodes = torch.unique(torch.cat([u, v]))
    blocks, input_ids = gcn_amd.sample_blocks(adj, nodes, fanouts, seed, offset + 1)
    return blocks, input_ids, torch.searchsorted(nodes, u), torch.searchsorted(nodes, v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rowptr, col, val, n = graphgen.make_graph("reddit", device=dev, seed=1, scale=args.scale)
    adj = gcn_amd.CsrAdjacency(rowptr, col, val, (n, n), symmetric=True)
    rows_of = _entry_rows(adj)
    keys = rows_of.long() * n + adj.col.long()             # ascending: the rows are column-sorted
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    res = {"graph": "reddit", "scale": args.scale, "n": n, "nnz": adj.nnz, "steps": args.steps, "warmup": args.warmup,
           "rounds": args.rounds,
           "what": "ms per call, wall clock ending in a synchronise; median and spread (max - min) over alternating rounds; "
                   "torch_*: the torch formulation on the same GPU", "cases": {}}
    ok = True

    # ---- every stored entry ----------------------------------------------------------------------------------------------------
    got = gcn_amd.find_edges(adj, rows_of, adj.col)        # (the first call checks the column order)
    want = torch_find(keys, n, rows_of, adj.col)
    row = {"queries": adj.nnz, "equals_torch": bool(torch.equal(got, want)), "found": int((got >= 0).sum())}
    ok = ok and row["equals_torch"] and row["found"] == adj.nnz
    few = max(2, min(args.steps, 5))
    row.update(alternate(lambda: gcn_amd.find_edges(adj, rows_of, adj.col), lambda: torch_find(keys, n, rows_of, adj.col),
                         few, 1, args.rounds))
    res["cases"]["find_edges_all_entries"] = row
    print(f"# {row}", file=sys.stderr, flush=True)

    # ---- 2^24 stored entries in random order (no two neighbouring lanes in one row) ---------------------------------------------
    pick = torch.randint(0, adj.nnz, (1 << 24,), device=dev, generator=gen)
    r_rows, r_cols = rows_of[pick], adj.col[pick]
    got = gcn_amd.find_edges(adj, r_rows, r_cols)
    row = {"queries": int(pick.numel()), "equals_torch": bool(torch.equal(got, torch_find(keys, n, r_rows, r_cols))),
           "found": int((got >= 0).sum())}
    ok = ok and row["equals_torch"] and row["found"] == pick.numel()
    row.update(alternate(lambda: gcn_amd.find_edges(adj, r_rows, r_cols), lambda: torch_find(keys, n, r_rows, r_cols),
                         args.steps, args.warmup, args.rounds))
    res["cases"]["find_edges_random_2e24"] = row
    print(f"# {row}", file=sys.stderr, flush=True)

    # ---- 2^20 negatives --------------------------------------------------------------------------------------------------------
    q = 1 << 20
    rows = torch.randint(0, n, (q,), device=dev, generator=gen)
    neg = gcn_amd.negative_sample(adj, rows, 1, seed=1, offset=0).reshape(-1)
    tneg = torch_negatives(keys, n, rows, gen)
    drawn = neg >= 0
    row = {"queries": q, "num_neg": 1, "max_tries": 32, "failed_slots": int((~drawn).sum()),
           "ours_valid": bool((torch_find(keys, n, rows[drawn], neg[drawn]) < 0).all()) and bool((neg != rows).all()),
           "torch_valid": bool((torch_find(keys, n, rows, tneg) < 0).all()) and bool((tneg != rows).all())}
    ok = ok and row["ours_valid"] and row["torch_valid"]
    row.update(alternate(lambda: gcn_amd.negative_sample(adj, rows, 1, seed=1, offset=0), lambda: torch_negatives(keys, n, rows, gen),
                         args.steps, args.warmup, args.rounds))
    res["cases"]["negative_sample_2e20"] = row
    print(f"# {row}", file=sys.stderr, flush=True)

    # ---- one loader batch ------------------------------------------------------------------------------------------------------
    batch, fanouts = 1024, [10, 5]
    eids = torch.randperm(adj.nnz, generator=torch.Generator().manual_seed(0))[:batch * 4].to(dev)
    loader = gcn_amd.LinkNeighborLoader(adj, eids, fanouts, batch, num_neg=1, shuffle=False, seed=1)
    blocks, input_ids, *_ = next(iter(loader))
    row = {"batch": batch, "num_neg": 1, "fanouts": fanouts, "input_vertices": int(input_ids.numel()),
           "seed_vertices": blocks[-1].num_dst}
    row.update(alternate(lambda: next(iter(loader)), lambda: torch_batch(adj, keys, eids[:batch], fanouts, gen, 1, 0),
                         args.steps, args.warmup, args.rounds))
    res["cases"]["link_loader_batch"] = row
    print(f"# {row}", file=sys.stderr, flush=True)

    res["error_check"] = "pass" if ok else "FAIL"
    line = json.dumps(res)
    print(line)
    out = args.out or os.path.join(ROOT, "profiles", "linkpred_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""The device merge (gcn_amd/coalesce.py, gcn_amd/csrc/coalesce.hip) against the torch formulation it replaces, on two
shapes: the Reddit-shaped graph (graphgen.make_graph("reddit"): one direction of every edge as a shuffled edge list, 57 M
edges) and a 50 000-seed fanout-10 block of it (its edges in the block's own vertex numbering, rows of at most 10 entries).
Self-loops are taken out of both lists and one edge in ten is repeated.  Per shape, ms per call:
  coalesce       gcn_amd.coalesce_csr(adj, "sum") on the CSR of the list (it sorts the columns itself)
                                                      vs  torch.sparse_coo_tensor(the same entries).coalesce()
  symmetrize     gcn_amd.symmetrize(merged, "sum")    vs  (S + S.t()).coalesce() on the merged COO matrix
  gcn_adjacency  gcn_amd.gcn_adjacency(rows, cols, n) vs  COO of the edges, their mirrors and the identity, .coalesce(), values
                                                          set to one, fp64 degrees by index_add, d^-1/2[r] * d^-1/2[c], to CSR
Every time is a host clock around `steps` calls that end in a device synchronise, `steps` chosen so that a window lasts
about 0.2 s.  The two sides of a comparison alternate, `--rounds` windows each: the median is reported, and the spread is
(max - min) / median of a side's windows.  `slower_beyond_spread` marks a comparison where the new median exceeds the old
one by more than the larger of the two spreads.  Results are checked equal first: patterns equal, merged values equal (the
values are eighths: sums are exact in any order), normalised values within one fp32 ulp.
`model_bytes` is the byte model of gcn_adjacency written out in DESIGN §4.15, evaluated for the shape.
Prints one JSON line and writes it to the profiles directory as coalesce_bench.json (--out FILE: elsewhere).

    python tools/coalesce_bench.py [--rounds 5] [--scale 1.0] [--seeds 50000] [--out FILE]
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


def window_ms(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def compare(new, old, rounds):
    """alternating windows of the two sides -> dict of medians, spreads and the verdict"""
    new(); old()                                           # warm-up: code objects, the allocator's blocks, the sort's choices
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


def entry_rows(adj):
    lens = (adj.rowptr[1:] - adj.rowptr[:-1]).long()
    return torch.repeat_interleave(torch.arange(adj.m, device=adj.device), lens, output_size=adj.nnz)


def coo_of(adj):
    return torch.sparse_coo_tensor(torch.stack([entry_rows(adj), adj.col.long()]), adj.val, (adj.m, adj.n))


def same_matrix(adj, coo, ulp=False):
    """a CsrAdjacency against a coalesced COO tensor: the pattern equal, the values equal or within one fp32 ulp"""
    r, c = coo.indices()
    ok = adj.nnz == r.numel() and bool(torch.equal(entry_rows(adj), r)) and bool(torch.equal(adj.col.long(), c))
    if not ok:
        return False
    if not ulp:
        return bool(torch.equal(adj.val, coo.values()))
    return bool(torch.all((adj.val - coo.values()).abs() <= 2.0 ** -23 * coo.values().abs()))


def torch_gcn_adjacency(rows, cols, n):
    """the formulation available without the merge: COO of the edges, the mirrors and the identity, coalesced; values one;
    degrees in fp64; D^-1/2 A D^-1/2 rounded to fp32 once; CSR"""
    loops = torch.arange(n, device=rows.device)
    idx = torch.stack([torch.cat([rows, cols, loops]), torch.cat([cols, rows, loops])])
    a = torch.sparse_coo_tensor(idx, torch.ones(idx.shape[1], device=rows.device), (n, n)).coalesce()
    r, c = a.indices()
    deg = torch.zeros(n, dtype=torch.float64, device=rows.device).index_add_(0, r, torch.ones(r.numel(), dtype=torch.float64,
                                                                                              device=rows.device))
    d = deg.pow(-0.5)
    d[torch.isinf(d)] = 0.0
    val = (d[r] * d[c]).float()
    return torch.sparse_coo_tensor(a.indices(), val, (n, n), is_coalesced=True), a.to_sparse_csr().crow_indices()


def model_bytes(E, T, Z, n):
    """the byte model of gcn_adjacency with its defaults: E edges (int64 ids), T = E + mirrors entries, Z
    entries of the result, n vertices; 4-byte words unless said"""
    mirrors = 2 * 8 * E + 2 * 4 * E + 2 * 4 * E + E + 8 * (T - E) + 2 * (8 + 4 + 4) * (T - E) + 2 * 2 * 4 * T
    sort = (5 + 3 + 5 + 3 + 3) * 4 * T + 2 * 4 * 4 * n
    merge = 2 * 4 * T + 4 * Z + 5 * 4 * n
    norm = 4 * n + 8 * n + 4 * Z + 8 * Z + 4 * Z
    return int(mirrors + sort + merge + norm)


def measure(name, rows, cols, n, rounds):
    """rows, cols: int64 device tensors, a directed edge list without self-loops"""
    dev = rows.device
    E = int(rows.numel())
    gen = torch.Generator(device="cpu")
    gen.manual_seed(5)
    vals = (torch.randint(1, 9, (E,), generator=gen).float() / 8).to(dev)
    adj, _ = gcn_amd.csr_from_edges(rows, cols, (n, n), vals)
    res = {"shape": name, "n": n, "edges": E, "longest_row": int((adj.rowptr[1:] - adj.rowptr[:-1]).max())}
    # ---- equal results first ---------------------------------------------------------------------------------------------
    merged, _ = gcn_amd.coalesce_csr(adj, "sum")
    old_merged = coo_of(adj).coalesce()
    ok = same_matrix(merged, old_merged)
    sym = gcn_amd.symmetrize(merged, "sum")
    ok = ok and same_matrix(sym, (old_merged + old_merged.t()).coalesce())
    a_hat = gcn_amd.gcn_adjacency(rows, cols, n)
    old_hat, old_crow = torch_gcn_adjacency(rows, cols, n)
    ok = ok and same_matrix(a_hat, old_hat, ulp=True) and bool(torch.equal(a_hat.rowptr.long(), old_crow))
    res.update(equal=ok, merged_nnz=merged.nnz, symmetrized_nnz=sym.nnz, a_hat_nnz=a_hat.nnz)
    mirrors = int((rows != cols).sum())
    res["model_bytes"] = model_bytes(E, E + mirrors, a_hat.nnz, n)
    del sym, a_hat, old_hat, old_crow
    # ---- times -----------------------------------------------------------------------------------------------------------
    coo = coo_of(adj)
    res["coalesce"] = compare(lambda: gcn_amd.coalesce_csr(adj, "sum"), lambda: coo.coalesce(), rounds)
    res["symmetrize"] = compare(lambda: gcn_amd.symmetrize(merged, "sum"), lambda: (old_merged + old_merged.t()).coalesce(), rounds)
    res["gcn_adjacency"] = compare(lambda: gcn_amd.gcn_adjacency(rows, cols, n), lambda: torch_gcn_adjacency(rows, cols, n), rounds)
    res["model_gb_per_s"] = round(res["model_bytes"] / (res["gcn_adjacency"]["new_ms"] * 1e-3) / 1e9, 1)
    return res


def edge_list(r, c, repeat=0.1, seed=3):
    """the edges shuffled, one in ten of them twice (int64 device tensors)"""
    gen = torch.Generator(device="cpu")
    gen.manual_seed(seed)
    extra = torch.randperm(r.numel(), generator=gen)[:int(repeat * r.numel())].to(r.device)
    r, c = torch.cat([r, r[extra]]), torch.cat([c, c[extra]])
    shuffle = torch.randperm(r.numel(), generator=gen).to(r.device)
    return r[shuffle], c[shuffle]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--seeds", type=int, default=50000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"rounds": args.rounds, "scale": args.scale,
           "what": "ms per call, median of `rounds` alternating windows of about 0.2 s (host clock, device synchronised); "
                   "new = gcn_amd.coalesce, old = the torch formulation named in the tool's header; spread = (max - min) / median",
           "shapes": []}
    rowptr, col, val, n = graphgen.make_graph("reddit", device=dev, seed=1, scale=args.scale)
    reddit = gcn_amd.CsrAdjacency(rowptr, col, val, (n, n), symmetric=False)
    gen = torch.Generator(device="cpu")
    gen.manual_seed(0)
    seeds = torch.randperm(n, generator=gen)[:min(args.seeds, n)].to(dev)
    blocks, _ = gcn_amd.sample_blocks(reddit, seeds, [10], seed=1, offset=0)
    b = blocks[0].adj
    br, bc = entry_rows(b), b.col.long()
    off = br != bc                                         # the block's edges in its own numbering, self-loops out
    shapes = [(f"block_{seeds.numel()}_seeds_fanout_10",) + edge_list(br[off], bc[off]) + (b.n,)]
    rr, rc = entry_rows(reddit), reddit.col.long()
    up = rr < rc                                           # one direction of every edge
    shapes.append(("reddit",) + edge_list(rr[up], rc[up]) + (n,))
    del br, bc, off, rr, rc, up
    del reddit, rowptr, col, val, blocks, b
    torch.cuda.empty_cache()
    ok = True
    for label, r, c, nv in shapes:
        row = measure(label, r, c, nv, args.rounds)
        ok = ok and row["equal"]
        res["shapes"].append(row)
        print(f"# {row}", file=sys.stderr, flush=True)
    res["error_check"] = "pass" if ok else "FAIL"
    line = json.dumps(res)
    print(line)
    out = args.out or os.path.join(ROOT, "profiles", "coalesce_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

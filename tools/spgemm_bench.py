#!/usr/bin/env python3
"""The device sparse x sparse product (gcn_amd/spgemm.py, gcn_amd/csrc/spgemm.hip) against torch.sparse.mm(S, S) on the
same device, on three workloads:
  hgnn_laplacian   the incidence matrix H of a 10-nearest-neighbour hypergraph on 232 965 vertices (one hyperedge per vertex:
                   itself and 10 random neighbours), G = L · Lᵀ with L = Dv^-1/2 H De^-1/2: gcn_amd.hypergraph_laplacian's
                   product, timed as spgemm(L, Lᵀ)      vs  torch.sparse.mm(L, Lᵀ) on sparse CSR tensors
  block_chain      the product of the two fanout-10 blocks sample_blocks yields for 50 000 seeds of the Reddit-shaped graph
                   (seeds x frontier · frontier x sources)
  two_hop          A · A on a random graph of mean degree 16 (2^18 vertices)
Per workload, ms per call: spgemm(a, b, assume_coalesced=True) against torch.sparse.mm(a, b).  Every time is a host clock
around `steps` calls that end in a device synchronise, `steps` chosen so that a window lasts about 0.2 s.  The two sides
alternate, `--rounds` windows each: the median is reported, and the spread is (max - min) / median of a side's windows.
Results are checked first: the patterns equal (values are positive, so torch drops nothing), and every value within
t * 2^-24 * sum |a b| of torch's, t the number of products of the entry — the summation bound of the tests, taken twice
because both sides carry it.
`model_bytes` is the byte model of count + fill written out in DESIGN §4.18, evaluated for the workload.
Prints one JSON line and writes it to the profiles directory as spgemm_bench.json (--out FILE: elsewhere).

    python tools/spgemm_bench.py [--rounds 5] [--scale 1.0] [--out FILE]
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
from coalesce_bench import compare, entry_rows  # noqa: E402


def torch_csr(adj, values=None):
    return torch.sparse_csr_tensor(adj.rowptr.long(), adj.col.long(), adj.val if values is None else values, (adj.m, adj.n))


def check(c, a, b):
    """c = spgemm(a, b) against torch.sparse.mm: the pattern, and the values within the summation bound"""
    ref = torch.sparse.mm(torch_csr(a), torch_csr(b))
    crow, ccol = ref.crow_indices(), ref.col_indices()
    order = None
    if not (c.nnz == ccol.numel() and bool(torch.equal(c.rowptr.long(), crow))):
        return False, None
    rows = entry_rows(c)
    key = rows * c.n + ccol                                # (torch's rows need not be column-sorted)
    order = torch.argsort(key)
    if not bool(torch.equal(ccol[order], c.col.long())):
        return False, None
    ones_a, ones_b = torch.ones_like(a.val), torch.ones_like(b.val)
    t = torch.sparse.mm(torch_csr(a, ones_a), torch_csr(b, ones_b)).values()[order]
    mag = torch.sparse.mm(torch_csr(a, a.val.abs()), torch_csr(b, b.val.abs())).values()[order]
    err = (c.val.double() - ref.values()[order].double()).abs()
    bound = 2.0 * t.double() * 2.0 ** -24 * mag.double()
    ratio = float((err / bound).max()) if c.nnz else 0.0
    return ratio <= 1.0, ratio


def model_bytes(a, b, c, products):
    """count + fill: both read A's row pointer, columns and the B row bounds of every entry of A twice (the
    product count, the walk) and B's columns of every product; the fill also reads A's values and B's values of every
    product; the count writes a length and a product count per row, the fill reads the scanned row pointer and writes the
    columns and values of C.  4-byte words"""
    walk = 2 * 4 * (a.m + 1) + 2 * (4 + 2 * 4) * a.nnz + 4 * products
    return int(2 * walk + 4 * a.nnz + 4 * products + 8 * a.m + 4 * a.m + 4 * (a.m + 1) + 8 * c.nnz)


def measure(name, a, b, rounds):
    lens_b = (b.rowptr[1:] - b.rowptr[:-1]).long()
    per_entry = lens_b[a.col.long()]
    products = int(per_entry.sum())
    per_row = torch.zeros(a.m, dtype=torch.int64, device=a.device).index_add_(0, entry_rows(a), per_entry)
    c = gcn_amd.spgemm(a, b, assume_coalesced=True)
    ok, ratio = check(c, a, b)
    W, G = gcn_amd._lib.SPGEMM_WAVE_MAX, gcn_amd._lib.SPGEMM_BLOCK_MAX
    k = torch.clamp(per_row, max=b.n)
    res = {"workload": name, "a": [a.m, a.n, a.nnz], "b": [b.m, b.n, b.nnz], "c_nnz": c.nnz, "products": products,
           "rows_wave": int((k <= W).sum()), "rows_block": int(((k > W) & (k <= G)).sum()), "rows_dense": int((k > G).sum()),
           "equal": bool(ok), "error_over_bound": ratio}
    ta, tb = torch_csr(a), torch_csr(b)
    res["spgemm"] = compare(lambda: gcn_amd.spgemm(a, b, assume_coalesced=True), lambda: torch.sparse.mm(ta, tb), rounds)
    res["model_bytes"] = model_bytes(a, b, c, products)
    res["model_gb_per_s"] = round(res["model_bytes"] / (res["spgemm"]["new_ms"] * 1e-3) / 1e9, 1)
    return res


def hypergraph_l(n, k, dev):
    """L = Dv^-1/2 H De^-1/2 for the hypergraph with one hyperedge per vertex: the vertex and k random neighbours"""
    gen = torch.Generator(device="cpu")
    gen.manual_seed(7)
    centre = torch.arange(n).repeat_interleave(k + 1)
    member = torch.randint(0, n, (n, k + 1), generator=gen)
    member[:, 0] = torch.arange(n)
    H, _ = gcn_amd.csr_from_edges(member.reshape(-1).to(dev), centre.to(dev), (n, n))
    H, _ = gcn_amd.coalesce_csr(H, "max", assume_sorted=True)              # (a neighbour drawn twice is one membership)
    rows = entry_rows(H)
    dv = torch.zeros(n, dtype=torch.float64, device=dev).index_add_(0, rows, H.val.double())
    de = torch.zeros(n, dtype=torch.float64, device=dev).index_add_(0, H.col.long(), H.val.double())
    lval = (H.val.double() / dv.sqrt()[rows] / de.sqrt()[H.col.long()]).float()
    return gcn_amd.CsrAdjacency(H.rowptr, H.col, lval, (n, n), symmetric=False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"rounds": args.rounds, "scale": args.scale,
           "what": "ms per call, median of `rounds` alternating windows of about 0.2 s (host clock, device synchronised); "
                   "new = gcn_amd.spgemm(a, b, assume_coalesced=True), old = torch.sparse.mm on sparse CSR tensors; "
                   "spread = (max - min) / median",
           "workloads": []}
    ok = True

    def run(name, a, b):
        nonlocal ok
        row = measure(name, a, b, args.rounds)
        ok = ok and row["equal"]
        res["workloads"].append(row)
        print(f"# {row}", file=sys.stderr, flush=True)

    L = hypergraph_l(max(1000, int(232965 * args.scale)), 10, dev)
    Lt, _ = gcn_amd.transpose_csr(L)
    run("hgnn_laplacian", L, Lt)
    g = gcn_amd.hypergraph_laplacian(L)                    # the whole call once: symmetric bit for bit on this shape too
    gt, _ = gcn_amd.transpose_csr(g)
    res["laplacian_equals_its_transpose"] = bool(torch.equal(g.col, gt.col) and torch.equal(g.val.view(torch.int32), gt.val.view(torch.int32)))
    ok = ok and res["laplacian_equals_its_transpose"]
    del L, Lt, g, gt
    torch.cuda.empty_cache()

    rowptr, col, val, n = graphgen.make_graph("reddit", device=dev, seed=1, scale=args.scale)
    reddit = gcn_amd.CsrAdjacency(rowptr, col, val, (n, n), symmetric=False)
    gen = torch.Generator(device="cpu")
    gen.manual_seed(0)
    seeds = torch.randperm(n, generator=gen)[:min(50000, n)].to(dev)
    blocks, _ = gcn_amd.sample_blocks(reddit, seeds, [10, 10], seed=1, offset=0)
    outer, inner = (blocks[0].adj, blocks[1].adj) if blocks[0].adj.m == blocks[1].adj.n else (blocks[1].adj, blocks[0].adj)
    run("block_chain", inner, outer)
    del reddit, rowptr, col, val, blocks, outer, inner
    torch.cuda.empty_cache()

    nv = max(1000, int((1 << 18) * args.scale))
    gen.manual_seed(1)
    r, c = torch.randint(0, nv, (16 * nv,), generator=gen).to(dev), torch.randint(0, nv, (16 * nv,), generator=gen).to(dev)
    vals = (0.5 + torch.rand(16 * nv, generator=gen)).to(dev)
    A, _ = gcn_amd.csr_from_edges(r, c, (nv, nv), vals)
    A, _ = gcn_amd.coalesce_csr(A, "sum", assume_sorted=True)
    run("two_hop", A, A)

    res["error_check"] = "pass" if ok else "FAIL"
    line = json.dumps(res)
    print(line)
    out = args.out or os.path.join(ROOT, "profiles", "spgemm_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""The product with a fixed pattern and its gradients (gcn_amd.SparseProduct, gcn_amd.HypergraphLaplacian: the sampled sparse
product of gcn_amd/csrc/sampled_dot.hip) on the three workloads of tools/spgemm_bench.py — hgnn_laplacian, block_chain,
two_hop.  Per workload, ms per call of
  spgemm            gcn_amd.spgemm(a, b, assume_coalesced=True) as it is: count + scan + the read of the total + fill
  values            SparseProduct.values(av, bv), no gradient asked for: one call of the kernel on C's pattern
  backward_a / _b / _ab   the backward of .values for a_values alone, b_values alone and both (the forward is not in the time)
  torch_fwd_bwd     torch.sparse.mm(S, S) on COO operands that require a gradient, forward + backward — or "unsupported" with
                    the error's text when this torch build refuses
and on hgnn_laplacian also hypergraph_laplacian(H, w) as it is against HypergraphLaplacian.values(w) forward and backward.
Every time is a host clock around `steps` calls that end in a device synchronise, `steps` chosen so that a window lasts about
0.2 s.  The sides alternate, `--rounds` windows each: the median is reported, and the spread is (max - min) / median of a side's
windows.  Checked first: .values equals spgemm's values bit for bit.
`model_bytes` evaluates the byte model of DESIGN §4.21 for the forward call.
Prints one JSON line and writes it to the profiles directory as spgemm_grad_bench.json (--out FILE: elsewhere).

    python tools/spgemm_grad_bench.py [--rounds 5] [--scale 1.0] [--out FILE]
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gcn_amd                                  # noqa: E402
from gcn_amd import graphgen                    # noqa: E402
from coalesce_bench import entry_rows, window_ms  # noqa: E402


def alternate(sides, rounds):
    """alternating windows of every side -> {name: {"ms": median, "spread": (max - min) / median, "steps": per window}}"""
    steps = {}
    for name, fn in sides.items():
        fn(); fn()                                         # warm-up: code objects, the allocator's blocks
        steps[name] = max(1, min(200, int(0.2 / max(window_ms(fn, 1) * 1e-3, 1e-6))))
    t = {name: [] for name in sides}
    for _ in range(rounds):
        for name, fn in sides.items():
            t[name].append(window_ms(fn, steps[name]))
    out = {}
    for name, v in t.items():
        med = statistics.median(v)
        out[name] = {"ms": round(med, 4), "spread": round((max(v) - min(v)) / med, 3), "steps": steps[name]}
    return out


def forward_model_bytes(P):
    """one call on C's pattern: C's row pointer and columns, per entry of C the two bounds of its Bᵀ row and
    that row's columns (what the searches of the entry touch), A's row once per row of C (columns and values: the groups'
    re-reads hit the L1), the two values of every match (a product of A · B), and the value written.  4-byte words.
    -> (bytes, entries of X visited = lookups)"""
    a, c, bt = P.a, P.adj, P.bt
    lens_a = (a.rowptr[1:] - a.rowptr[:-1]).long()
    lens_b = (P.b.rowptr[1:] - P.b.rowptr[:-1]).long()
    lens_bt = (bt.rowptr[1:] - bt.rowptr[:-1]).long()
    work = int((lens_a * (c.rowptr[1:] - c.rowptr[:-1]).long()).sum())
    products = int(lens_b[a.col.long()].sum())
    y_cols = int(lens_bt[c.col.long()].sum())
    return int(4 * (c.m + 1) + 4 * c.nnz + 8 * c.nnz + 4 * y_cols + 8 * a.nnz + 8 * products + 4 * c.nnz), work


def torch_side(a, b):
    """forward + backward of torch.sparse.mm on COO operands that require a gradient, or the reason it cannot be timed"""
    def coo(x):
        return torch.sparse_coo_tensor(torch.stack([entry_rows(x), x.col.long()]), x.val, (x.m, x.n)).coalesce()
    try:
        ta, tb = coo(a).requires_grad_(True), coo(b).requires_grad_(True)

        def fn():
            ta.grad = tb.grad = None
            torch.sparse.sum(torch.sparse.mm(ta, tb)).backward()
        fn()
        torch.cuda.synchronize()
        return fn, None
    except Exception as e:                                 # noqa: BLE001 (whatever this build raises is the finding)
        return None, f"unsupported: {type(e).__name__}: {str(e)[:200]}"


def measure(name, a, b, rounds):
    P = gcn_amd.SparseProduct(a, b)
    c = gcn_amd.spgemm(a, b, assume_coalesced=True)
    equal = bool(torch.equal(c.col, P.adj.col) and torch.equal(P.values().view(torch.int32), c.val.view(torch.int32)))
    g = torch.ones(P.adj.nnz, device=a.device)
    need = {"backward_a": (True, False), "backward_b": (False, True), "backward_ab": (True, True)}
    sides = {"spgemm": lambda: gcn_amd.spgemm(a, b, assume_coalesced=True), "values": lambda: P.values(a.val, b.val)}
    for key, (na, nb) in need.items():
        av, bv = a.val.clone().requires_grad_(na), b.val.clone().requires_grad_(nb)
        v = P.values(av, bv)
        inputs = tuple(x for x, n in ((av, na), (bv, nb)) if n)
        sides[key] = (lambda v=v, inputs=inputs: torch.autograd.grad(v, inputs, g, retain_graph=True))
    fn, why = torch_side(a, b)
    if fn is not None:
        sides["torch_fwd_bwd"] = fn
    res = {"workload": name, "a": [a.m, a.n, a.nnz], "b": [b.m, b.n, b.nnz], "c_nnz": P.adj.nnz, "values_equal_spgemm": equal}
    res.update(alternate(sides, rounds))
    if fn is None:
        res["torch_fwd_bwd"] = why
    res["model_bytes"], res["x_entries_visited"] = forward_model_bytes(P)
    res["model_gb_per_s"] = round(res["model_bytes"] / (res["values"]["ms"] * 1e-3) / 1e9, 1)
    res["refresh_over_spgemm"] = round(res["spgemm"]["ms"] / res["values"]["ms"], 2)
    return res, equal


def hypergraph_h(n, k, dev):
    """H of the hypergraph with one hyperedge per vertex, the vertex and k random neighbours (tools/spgemm_bench.py's)"""
    gen = torch.Generator(device="cpu")
    gen.manual_seed(7)
    centre = torch.arange(n).repeat_interleave(k + 1)
    member = torch.randint(0, n, (n, k + 1), generator=gen)
    member[:, 0] = torch.arange(n)
    H, _ = gcn_amd.csr_from_edges(member.reshape(-1).to(dev), centre.to(dev), (n, n))
    H, _ = gcn_amd.coalesce_csr(H, "max", assume_sorted=True)              # (a neighbour drawn twice is one membership)
    return H


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"rounds": args.rounds, "scale": args.scale,
           "what": "ms per call, median of `rounds` alternating windows of about 0.2 s (host clock, device synchronised); "
                   "spread = (max - min) / median; backward_*: the backward alone",
           "workloads": []}
    ok = True

    def run(name, a, b):
        nonlocal ok
        row, equal = measure(name, a, b, args.rounds)
        ok = ok and equal
        res["workloads"].append(row)
        print(f"# {row}", file=sys.stderr, flush=True)

    n = max(1000, int(232965 * args.scale))
    H = hypergraph_h(n, 10, dev)
    lap = gcn_amd.HypergraphLaplacian(H)
    run("hgnn_laplacian", lap.product.a, lap.product.b)
    gen = torch.Generator(device="cpu")
    gen.manual_seed(3)
    w = (0.5 + torch.rand(n, generator=gen)).to(dev)
    same = bool(torch.equal(lap.values(w).view(torch.int32), gcn_amd.hypergraph_laplacian(H, w).val.view(torch.int32)))
    ok = ok and same
    wg = w.clone().requires_grad_(True)
    v = lap.values(wg)
    g = torch.ones_like(v)
    res["laplacian"] = {"values_equal_hypergraph_laplacian": same}
    res["laplacian"].update(alternate({"hypergraph_laplacian": lambda: gcn_amd.hypergraph_laplacian(H, w),
                                       "values": lambda: lap.values(w),
                                       "backward": lambda: torch.autograd.grad(v, wg, g, retain_graph=True)}, args.rounds))
    print(f"# {res['laplacian']}", file=sys.stderr, flush=True)
    del H, lap, v, g, wg
    torch.cuda.empty_cache()

    rowptr, col, val, n = graphgen.make_graph("reddit", device=dev, seed=1, scale=args.scale)
    reddit = gcn_amd.CsrAdjacency(rowptr, col, val, (n, n), symmetric=False)
    gen.manual_seed(0)
    seeds = torch.randperm(n, generator=gen)[:min(50000, n)].to(dev)
    blocks, _ = gcn_amd.sample_blocks(reddit, seeds, [10, 10], seed=1, offset=0)
    outer, inner = (blocks[0].adj, blocks[1].adj) if blocks[0].adj.m == blocks[1].adj.n else (blocks[1].adj, blocks[0].adj)
    outer, _ = gcn_amd.coalesce_csr(outer, "sum")          # (SparseProduct wants b's rows ascending)
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
    out = args.out or os.path.join(ROOT, "profiles", "spgemm_grad_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

"""One-pass multi-aggregation on the GPU (gcn_amd/csrc/aggregate_multi.hip, gcn_amd.aggregate_multi, PNAConv).

References are fp64, written plainly per row on the gathered slab x[col[b:e]]: numpy's sum / mean / var, np.argmax /
np.argmin (the kernel's selection rule, so max / min are compared BY BITS and the args for equality).  Bounds: sums
1e-5 * sum|x| (the project's figure for fp32 sums; the mean the same over n_r); var 1e-5 * range^2 with range the fp64
max - min of the row's column — the shifted sums stay below 2e-7 * range^2, while sum(x^2) - sum(x)^2 / n misses by 0.05
* range^2 on features 1000 + U(-1, 1); std through its square, plus 4 ulp of (var + eps) for the addition and the root.
Gradients 1e-5 * the sum of the absolute terms, the layer 1e-4 relative."""
import numpy as np
import pytest
import torch

import gcn_amd
from test_aggregate_gpu import bits, graph, make_adj
from util import offset_view

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ALL = ("max", "min", "sum", "mean", "var", "std")
EPS = 1e-5
EPS32 = float(np.float32(EPS))


def features(n, k, seed):
    return (1000.0 + np.random.default_rng(seed).uniform(-1, 1, (n, k))).astype(np.float32)


def ref_rows(rp, col, x):
    """name -> [m, k] per row in fp64 (max / min fp32 with their int32 args; "abs" = sum|x|, "range" = max - min)"""
    m, k = len(rp) - 1, x.shape[1]
    R = {name: np.zeros((m, k)) for name in ("sum", "mean", "var", "abs", "range")}
    R.update({name: np.zeros((m, k), np.float32) for name in ("max", "min")})
    R.update({name: np.full((m, k), -1, np.int32) for name in ("argmax", "argmin")})
    jj = np.arange(k)
    for r in range(m):
        b, e = int(rp[r]), int(rp[r + 1])
        if e == b:
            continue
        slab = x[col[b:e]]
        s64 = slab.astype(np.float64)
        with np.errstate(all="ignore"):
            R["sum"][r], R["mean"][r], R["var"][r], R["abs"][r] = s64.sum(0), s64.mean(0), s64.var(0), np.abs(s64).sum(0)
            R["range"][r] = s64.max(0) - s64.min(0)
        for name, pick in (("max", np.argmax), ("min", np.argmin)):
            a = pick(slab, axis=0)
            R[name][r], R["arg" + name][r] = slab[a, jj], b + a
    return R


def planes(out, reduce):
    k = out.shape[1] // len(reduce)
    return {name: out[:, p * k:(p + 1) * k] for p, name in enumerate(reduce)}


@pytest.mark.parametrize("k", [1, 4, 65, 68])          # the element path, one vector, a tail tile on each path
@pytest.mark.parametrize("name", ["boundaries", "rect", "one_row"])
def test_forward_matches_fp64_per_row(name, k):
    rp, col, n = graph(name)
    x = features(n, k, seed=k)
    out, argmax, argmin = gcn_amd.aggregate_multi(make_adj(name), torch.from_numpy(x).to(DEV), ALL, EPS, return_arg=True)
    assert out.shape == (len(rp) - 1, 6 * k) and out.dtype == torch.float32 and argmax.dtype == torch.int32
    check_planes(out.cpu().numpy(), argmax, argmin, rp, ref_rows(rp, col, x), f"{name} k={k}")


def check_planes(out, argmax, argmin, rp, R, what):        # out: numpy, the six planes in ALL's order; R: ref_rows'
    P = planes(out, ALL)
    for op, arg in (("max", argmax), ("min", argmin)):
        assert np.array_equal(arg.cpu().numpy(), R["arg" + op]), op
        assert np.array_equal(bits(P[op]), bits(R[op])), op
    lens = np.diff(rp)[:, None]
    nr, full = np.maximum(lens, 1), lens > 0
    var_eps = R["var"] + EPS32
    excess = {"sum": np.abs(P["sum"] - R["sum"]) - (1e-5 * R["abs"] + 1e-30),
              "mean": np.abs(P["mean"] - R["mean"]) - (1e-5 * R["abs"] / nr + 1e-30),
              "var": np.abs(P["var"] - R["var"]) - 1e-5 * R["range"] ** 2,
              "std": (np.abs(P["std"].astype(np.float64) ** 2 - var_eps) - (1e-5 * R["range"] ** 2 + 4 * 2.0 ** -24 * var_eps)) * full}
    for name, ex in excess.items():
        print(f"[aggregate_multi] {what} {name}: max |err| - bound = {ex.max():.3e}")
        assert ex.max() <= 0, (name, float(ex.max()))
    assert (out[~full[:, 0]] == 0).all()                # empty rows: zeros in every plane, std included


@pytest.mark.parametrize("reduce", [("std",), ("max", "sum"), ALL[::-1]])
def test_planes_are_those_of_the_full_call_bit_for_bit(reduce):
    adj = make_adj("boundaries")
    x = torch.from_numpy(features(adj.n, 8, seed=1)).to(DEV)
    full = planes(gcn_amd.aggregate_multi(adj, x, ALL, EPS), ALL)
    out, argmax, argmin = gcn_amd.aggregate_multi(adj, x, reduce, EPS, return_arg=True)
    assert out.shape == (adj.m, len(reduce) * 8) and not out.requires_grad and out.grad_fn is None    # (a frozen x: no backward)
    assert (argmax is None) == ("max" not in reduce) and (argmin is None) == ("min" not in reduce)
    for name, plane in planes(out, reduce).items():
        assert np.array_equal(bits(plane), bits(full[name])), name


def test_empty_single_and_constant_rows_are_exact_and_a_misaligned_x_gives_the_same_bits():
    lens = np.array([0, 1, 5000, 0, 3, 1], np.int64)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    col = np.random.default_rng(0).integers(0, 10, rp[-1]).astype(np.int32)
    col[1:5001] = 7                                     # row 2: 5 000 copies of one column
    adj = gcn_amd.CsrAdjacency(torch.from_numpy(rp).to(DEV), torch.from_numpy(col).to(DEV), torch.ones(len(col), device=DEV), (6, 10))
    x = torch.from_numpy(features(10, 8, seed=2))
    out, argmax, argmin = gcn_amd.aggregate_multi(adj, x.to(DEV), ALL, EPS, return_arg=True)
    P = planes(out, ALL)
    empty, const = [0, 3], [1, 2, 5]
    assert (out[empty] == 0).all() and (argmax[empty] == -1).all() and (argmin[empty] == -1).all()
    assert (P["var"][const] == 0).all() and (P["std"][const] == float(np.sqrt(np.float32(EPS)))).all()
    assert torch.equal(P["max"][2], x[7].to(DEV)) and (argmax[2] == 1).all() and (argmin[2] == 1).all()
    shifted, _flat = offset_view(x, 1, torch.float32, DEV)
    out1, argmax1, argmin1 = gcn_amd.aggregate_multi(adj, shifted, ALL, EPS, return_arg=True)
    assert np.array_equal(bits(out1), bits(out)) and torch.equal(argmax1, argmax) and torch.equal(argmin1, argmin)


def test_non_finite_entries_give_numpys_pattern_and_leave_other_rows_alone():
    rp, col, n = graph("rect")
    adj = make_adj("rect")
    x = features(n, 4, seed=3)
    clean = gcn_amd.aggregate_multi(adj, torch.from_numpy(x).to(DEV), ALL, EPS).cpu().numpy()
    long_row = int(np.argmax(np.diff(rp)))
    cp, cm, cn = (int(c) for c in np.unique(col[rp[long_row]:rp[long_row + 1]])[:3])    # one row lists all three
    x[cp], x[cm], x[cn] = np.inf, -np.inf, np.nan
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    hit = {c: np.isin(np.arange(len(rp) - 1), rows[col == c]) for c in (cp, cm, cn)}
    assert (hit[cp] & ~hit[cm] & ~hit[cn]).any() and (hit[cm] & ~hit[cp] & ~hit[cn]).any() and (hit[cp] & hit[cm]).any()
    got = planes(gcn_amd.aggregate_multi(adj, torch.from_numpy(x).to(DEV), ALL, EPS).cpu().numpy(), ALL)
    R = ref_rows(rp, col, x)
    with np.errstate(all="ignore"):
        R["std"] = np.where(np.diff(rp)[:, None] > 0, np.sqrt(R["var"] + EPS32), 0.0)
    for name in ALL:
        for kind in (np.isnan, np.isposinf, np.isneginf):
            assert np.array_equal(kind(got[name]), kind(R[name])), (name, kind.__name__)
    untouched = ~(hit[cp] | hit[cm] | hit[cn])
    assert untouched.sum() > 100 and np.array_equal(bits(np.concatenate([got[name] for name in ALL], 1)[untouched]), bits(clean[untouched]))


def ref_gradient(rp, col, n, x64, g, argmax, argmin, magnitude):
    """gx in fp64 from the formula, entry by entry (magnitude: with |g| and |x - mean|, the sum of the absolute terms)"""
    m, k = len(rp) - 1, x64.shape[1]
    lens = torch.from_numpy(np.diff(rp).astype(np.int64))
    rows, c = torch.repeat_interleave(torch.arange(m), lens), torch.from_numpy(col.astype(np.int64))
    nr = lens.clamp(min=1).double()[:, None]
    mean = torch.zeros(m, k, dtype=torch.float64).index_add_(0, rows, x64[c]) / nr
    std = (torch.zeros(m, k, dtype=torch.float64).index_add_(0, rows, (x64[c] - mean[rows]) ** 2) / nr + EPS32).sqrt()
    G = {name: (p.abs() if magnitude else p) for name, p in planes(g.double(), ALL).items()}
    dev = x64[c] - mean[rows]
    dev = dev.abs() if magnitude else dev
    term = G["sum"][rows] + (G["mean"] / nr)[rows] + (2 * G["var"] / nr)[rows] * dev + (G["std"] / (nr * std))[rows] * dev
    gx = torch.zeros(n, k, dtype=torch.float64).index_add_(0, c, term)
    jj = torch.arange(k).expand(m, k)
    for name, arg in (("max", argmax), ("min", argmin)):
        ok = arg >= 0
        gx.index_put_((c[arg[ok].long()], jj[ok]), G[name][ok], accumulate=True)
    return gx


@pytest.mark.parametrize("k", [3, 64])
@pytest.mark.parametrize("name", ["rect", "boundaries_T"])
def test_backward_matches_the_fp64_formula(name, k):
    rp, col, n = graph(name)
    adj = make_adj(name)
    gen = torch.Generator().manual_seed(k)
    x = torch.randn(n, k, generator=gen)
    g = torch.randn(adj.m, 6 * k, generator=gen)
    xd = x.to(DEV).requires_grad_(True)
    out, argmax, argmin = gcn_amd.aggregate_multi(adj, xd, ALL, EPS, return_arg=True)
    (gx,) = torch.autograd.grad(out, xd, g.to(DEV))
    ref, mag = (ref_gradient(rp, col, n, x.double(), g, argmax.cpu(), argmin.cpu(), magnitude) for magnitude in (False, True))
    excess = (gx.cpu().double() - ref).abs() - (1e-5 * mag + 1e-30)
    print(f"[aggregate_multi] {name} k={k} grad x: max |err| - bound = {excess.max():.3e}, max err / terms = "
          f"{((gx.cpu().double() - ref).abs() / mag.clamp(min=1e-300)).max():.2e}")
    assert gx.shape == (n, k) and excess.max() <= 0, float(excess.max())


def test_forward_backward_captures_and_replays_bit_for_bit():
    adj = make_adj("boundaries")
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(adj.n, 8, generator=gen).to(DEV).requires_grad_(True)
    gout = torch.randn(adj.m, 48, generator=gen).to(DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                      # one eager call: the workspace, the transpose and its permutation exist
        gcn_amd.aggregate_multi(adj, x, ALL).backward(gout)
    torch.cuda.current_stream().wait_stream(side)
    x.grad = None
    graph_ = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph_):
        out = gcn_amd.aggregate_multi(adj, x, ALL)
        out.backward(gout)
    for _rep in range(2):
        with torch.no_grad():
            x.copy_(torch.randn(adj.n, 8, generator=gen).to(DEV))
            gout.copy_(torch.randn(adj.m, 48, generator=gen).to(DEV))
        graph_.replay()
        torch.cuda.synchronize()
        xe = x.detach().clone().requires_grad_(True)
        oe = gcn_amd.aggregate_multi(adj, xe, ALL)
        oe.backward(gout)
        assert np.array_equal(bits(out), bits(oe)) and np.array_equal(bits(x.grad), bits(xe.grad))


def pna64(x_src, x_dst, rp, col, layer, weight, bias):
    """the layer's composition in fp64 torch, differentiable"""
    m, k = len(rp) - 1, x_src.shape[1]
    lens = torch.from_numpy(np.diff(rp).astype(np.int64))
    rows, c = torch.repeat_interleave(torch.arange(m), lens), torch.from_numpy(col.astype(np.int64))
    nr, slab = lens.clamp(min=1).double()[:, None], x_src[c]
    zero = torch.zeros(m, k, dtype=torch.float64)
    mean = zero.index_add(0, rows, slab) / nr
    var = zero.index_add(0, rows, (slab - mean[rows]) ** 2) / nr
    at = rows[:, None].expand(-1, k)
    stat = {"mean": mean, "std": torch.where(lens[:, None] > 0, (var + layer.eps).sqrt(), zero),
            "max": zero.scatter_reduce(0, at, slab, "amax", include_self=False),
            "min": zero.scatter_reduce(0, at, slab, "amin", include_self=False)}
    h = torch.cat([stat[a] for a in layer.aggregators], 1)
    s = torch.log1p(lens.double())[:, None] / layer.delta
    return torch.cat([x_dst, h, h * s, h * torch.where(s > 0, 1 / s, torch.zeros_like(s))], 1) @ weight + bias


@pytest.mark.parametrize("sampled", [False, True])
def test_pna_conv_matches_the_fp64_composition(sampled):
    rp, col, n = graph("cora")
    adj = make_adj("cora")
    torch.manual_seed(3)
    layer = gcn_amd.PNAConv(16, 8, avg_log_degree=gcn_amd.PNAConv.avg_log_degree(adj)).to(DEV)
    assert abs(layer.delta - np.log1p(np.diff(rp)).mean()) <= 1e-6 * layer.delta
    x = torch.randn(n, 16)
    if sampled:
        (blk,), ids = gcn_amd.sample_blocks(adj, torch.arange(0, n, 5, device=DEV), [4], seed=1)
        adj, x = blk.adj, x[ids.cpu().long()]
        rp, col = adj.rowptr.cpu().numpy(), adj.col.cpu().numpy()
    xd = x.to(DEV).requires_grad_(True)
    out = layer((xd, xd[:adj.m]) if sampled else xd, adj)
    gout = torch.randn(adj.m, 8)
    out.backward(gout.to(DEV))
    x64, w64, b64 = (t.detach().cpu().double().requires_grad_(True) for t in (x, layer.weight, layer.bias))
    ref = pna64(x64, x64[:adj.m], rp, col, layer, w64, b64)
    ref.backward(gout.double())
    for what, got, want in (("out", out, ref), ("grad x", xd.grad, x64.grad), ("grad weight", layer.weight.grad, w64.grad),
                            ("grad bias", layer.bias.grad, b64.grad)):
        rel = float((got.detach().cpu().double() - want.detach()).abs().max() / want.detach().abs().max())
        print(f"[aggregate_multi] PNAConv sampled={sampled} {what}: relative error {rel:.2e}")
        assert rel <= 1e-4, (what, rel)

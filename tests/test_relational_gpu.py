"""Relation-typed aggregation on the GPU (gcn_amd/csrc/relational.hip, gcn_amd.relation_aggregate, EdgeTypes, RGCNConv).

References are plain fp64 numpy on the entry list: a loop over the planes with np.add.at, a masked entry simply left
out.  Bounds: every sum and gradient 1e-5 * the sum of the absolute terms (the project's figure for fp32 sums in a fixed
order, test_aggregate_multi_gpu.py), the layer 1e-4 relative against a per-relation fp64 torch formulation.  Types are
drawn uniformly with a fixed seed; with masks, uniformly from [-1, R], both ends out of range."""
import importlib

import numpy as np
import pytest
import torch

import gcn_amd
import test_autograd_forms_gpu as forms
from test_aggregate_gpu import bits, graph, make_adj

_relational = importlib.import_module("gcn_amd.relational")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MODES = {"typed3": (3, None), "R5B2": (5, 2), "R4B9": (4, 9)}          # name -> (R, B); B = 9: two passes, a one-plane tail


def entries(name, R, seed, masks=False):
    """(rows, col, etype int32, values fp32, n) of the graph, one element per stored entry"""
    rp, col, n = graph(name)
    rng = np.random.default_rng(seed)
    et = rng.integers(-1 if masks else 0, R + 1 if masks else R, len(col)).astype(np.int32)
    return np.repeat(np.arange(len(rp) - 1), np.diff(rp)), col, et, rng.uniform(0.5, 1.5, len(col)).astype(np.float32), n


def operands(n, k, R, B, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, k)).astype(np.float32), None if B is None else rng.standard_normal((R, B)).astype(np.float32)


def weights(et, val, coeff, R, b):
    """w(e, b) in fp64 for entries whose types lie in [0, R)"""
    return val * ((et == b) if coeff is None else coeff[et, b].astype(np.float64))


def ref_forward(rows, col, et, val, x, coeff, R, m):
    """(Y, sum of |terms|), fp64 [m, B k]; entries with a type outside [0, R) are REMOVED first"""
    keep = (et >= 0) & (et < R)
    rows, col, et, val = rows[keep], col[keep], et[keep], val[keep].astype(np.float64)
    B, k = R if coeff is None else coeff.shape[1], x.shape[1]
    Y, M = np.zeros((m, B, k)), np.zeros((m, B, k))
    for b in range(B):
        term = weights(et, val, coeff, R, b)[:, None] * x[col].astype(np.float64)
        np.add.at(Y[:, b], rows, term)
        np.add.at(M[:, b], rows, np.abs(term))
    return Y.reshape(m, -1), M.reshape(m, -1)


def within(got, ref, mag, what):
    excess = np.abs(got.detach().cpu().numpy().astype(np.float64) - ref) - (1e-5 * mag + 1e-30)
    print(f"[relational] {what}: max |err| - bound = {excess.max():.3e}")
    assert got.shape == ref.shape and excess.max() <= 0, (what, float(excess.max()))


def dev(a, grad=False):
    return None if a is None else torch.from_numpy(a).to(DEV).requires_grad_(grad)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("k", [1, 4, 65, 68])          # the element path, one vector, a tail tile on each path
@pytest.mark.parametrize("name", ["boundaries", "rect"])
def test_forward_matches_fp64_and_repeats(name, k, mode):
    R, B = MODES[mode]
    rows, col, et, val, n = entries(name, R, seed=k)
    adj = make_adj(name)
    x, coeff = operands(n, k, R, B, seed=k + 1)
    types = gcn_amd.EdgeTypes(adj, dev(et), R)
    out = gcn_amd.relation_aggregate(types, dev(x), dev(coeff), dev(val))
    ref, mag = ref_forward(rows, col, et, val, x, coeff, R, adj.m)
    within(out, ref, mag, f"forward {name} k={k} {mode}")
    assert (out[torch.from_numpy(np.bincount(rows, minlength=adj.m) == 0).to(DEV)] == 0).all()     # empty rows, every plane
    assert np.array_equal(bits(gcn_amd.relation_aggregate(types, dev(x), dev(coeff), dev(val))), bits(out))


def test_out_of_range_types_are_masks():
    R, B, k = 5, 2, 8
    rows, col, et, val, n = entries("rect", R, seed=3, masks=True)
    assert (et == -1).sum() > 100 and (et == R).sum() > 100
    adj = make_adj("rect")
    x, coeff = operands(n, k, R, B, seed=4)
    out = gcn_amd.relation_aggregate(gcn_amd.EdgeTypes(adj, dev(et), R), dev(x), dev(coeff), dev(val))
    within(out, *ref_forward(rows, col, et, val, x, coeff, R, adj.m), "forward rect with masked entries")


def test_typed_mode_keeps_a_nan_row_inside_its_relation():
    R, k = 3, 4
    rows, col, et, val, n = entries("rect", R, seed=5)
    adj = make_adj("rect")
    c = int(col[0])
    et[col == c] = 0                                    # column c is listed by entries of relation 0 only
    x, _ = operands(n, k, R, None, seed=6)
    x[c] = np.nan
    out = gcn_amd.relation_aggregate(gcn_amd.EdgeTypes(adj, dev(et), R), dev(x), None, dev(val)).cpu().numpy()
    listing = np.isin(np.arange(adj.m), rows[col == c])
    assert listing.any() and not listing.all()
    assert np.array_equal(np.isnan(out[:, :k]), np.repeat(listing[:, None], k, 1)) and np.isfinite(out[:, k:]).all()


@pytest.mark.parametrize("k,mode", [(4, "R5B2"), (65, "R5B2"), (4, "R4B9"), (65, "R4B9"), (65, "typed3")])
@pytest.mark.parametrize("name", ["boundaries_T", "rect"])          # hub columns in the transposed walk
def test_backward_x_matches_fp64_and_repeats(name, k, mode):
    R, B = MODES[mode]
    rows, col, et, val, n = entries(name, R, seed=k, masks=True)
    adj = make_adj(name)
    x, coeff = operands(n, k, R, B, seed=k + 1)
    planes = R if B is None else B
    g = np.random.default_rng(k + 2).standard_normal((adj.m, planes * k)).astype(np.float32)
    types, xd = gcn_amd.EdgeTypes(adj, dev(et), R), dev(x, grad=True)
    grad = lambda: torch.autograd.grad(gcn_amd.relation_aggregate(types, xd, dev(coeff), dev(val)), xd, dev(g))[0]
    gx = grad()
    keep = (et >= 0) & (et < R)
    ref, mag = np.zeros((n, k)), np.zeros((n, k))
    g3 = g.astype(np.float64).reshape(adj.m, planes, k)
    for b in range(planes):
        term = weights(et[keep], val[keep].astype(np.float64), coeff, R, b)[:, None] * g3[rows[keep], b]
        np.add.at(ref, col[keep], term)
        np.add.at(mag, col[keep], np.abs(term))
    within(gx, ref, mag, f"grad x {name} k={k} {mode}")
    assert np.array_equal(bits(grad()), bits(gx))


@pytest.mark.parametrize("k", [4, 65])
@pytest.mark.parametrize("name,R,B", [("boundaries", 3, 3), ("rect", 300, 9)])    # long relations (chunk merge); short and empty ones
def test_backward_coeff_matches_fp64_and_repeats(name, R, B, k):
    rows, col, et, val, n = entries(name, R, seed=k, masks=True)
    et[(et >= 280) & (et < R)] = -1                     # R = 300: relations 280 .. 299 are empty
    keep = (et >= 0) & (et < R)
    counts = np.bincount(et[keep], minlength=R)
    assert counts.min() > 4096 if R == 3 else (counts[:280].min() > 0 and counts[280:].max() == 0)
    adj = make_adj(name)
    x, coeff = operands(n, k, R, B, seed=k + 1)
    g = np.random.default_rng(k + 2).standard_normal((adj.m, B * k)).astype(np.float32)
    types, cd = gcn_amd.EdgeTypes(adj, dev(et), R), dev(coeff, grad=True)
    grad = lambda: torch.autograd.grad(gcn_amd.relation_aggregate(types, dev(x), cd, dev(val)), cd, dev(g))[0]
    gc = grad()
    ref, mag = np.zeros((R, B)), np.zeros((R, B))
    xs, g3 = x[col[keep]].astype(np.float64), g.astype(np.float64).reshape(adj.m, B, k)
    for b in range(B):
        term = val[keep].astype(np.float64)[:, None] * xs * g3[rows[keep], b]
        np.add.at(ref[:, b], et[keep], term.sum(1))
        np.add.at(mag[:, b], et[keep], np.abs(term).sum(1))
    within(gc, ref, mag, f"grad coeff {name} R={R} B={B} k={k}")
    assert (gc[torch.from_numpy(counts == 0).to(DEV)] == 0).all() and np.array_equal(bits(grad()), bits(gc))


# ---- the autograd contract (tests/autograd_forms.py) on _RelationFunction: the specs are entered into the SPECS of
# tests/test_autograd_forms_gpu.py on import, where tests/test_autograd_forms_cpu.py reads them (as the edge_aggregate and
# aggregate_multi form files do); small integers, so every sum is exact in any order and fp64 gives the same bits
def relation_specs():
    P = forms.pattern("rect")
    specs = []
    for name, R, B, k in (("relation_aggregate R=4 B=3 k=5", 4, 3, 5), ("relation_aggregate typed R=3 k=64", 3, None, 64)):
        rng = np.random.default_rng(R)
        et, val = rng.integers(-1, R + 1, P.nnz), rng.integers(1, 3, P.nnz).astype(np.float32)
        keep = np.flatnonzero((et >= 0) & (et < R))

        def make(seed, device, R=R, B=B, k=k):
            ops = [forms.ints((P.n, k), 60 * seed + k, 4, device)] + ([forms.ints((R, B), 60 * seed + k + 1, 2, device)] if B else [])
            return ops, forms.ints((P.m, (B or R) * k), 60 * seed + k + 2, 4, device)

        def reference(x, coeff=None, R=R, et=et, val=val, keep=keep):
            row, col = (t[torch.from_numpy(keep).to(x.device)] for t in P.index(x.device))
            t, v = torch.from_numpy(et[keep]).to(x.device), torch.from_numpy(val[keep]).to(device=x.device, dtype=x.dtype)
            w = (coeff[t] if coeff is not None else torch.nn.functional.one_hot(t, R).to(x.dtype)) * v[:, None]       # [entries, planes]
            return torch.zeros(P.m, w.shape[1], x.shape[1], dtype=x.dtype, device=x.device).index_add(
                0, row, w[:, :, None] * x[col][:, None, :]).reshape(P.m, -1)

        def build(name=name, R=R, et=et, val=val):
            types, v = gcn_amd.EdgeTypes(P.adj(name), dev(et.astype(np.int32)), R), dev(val)
            return (lambda x, coeff=None: gcn_amd.relation_aggregate(types, x, coeff, v)), None
        specs.append(forms.Spec(name, [_relational._RelationFunction], make, reference, build))
    return specs


REL_SPECS = relation_specs()
REL_IDS = [s.name.replace(" ", "_") for s in REL_SPECS]
if not any(s.name == REL_SPECS[0].name for s in forms.SPECS):
    forms.SPECS = forms.SPECS + REL_SPECS                  # (a new list: that module's own parametrisation keeps its own)


@pytest.mark.parametrize("spec", REL_SPECS, ids=REL_IDS)
def test_the_canonical_call_matches_fp64_autograd_of_the_plain_formulation(spec):
    forms.test_the_canonical_call_matches_fp64_autograd_of_the_plain_formulation(spec)


@pytest.mark.parametrize("form", list(forms.af.FORMS), ids=[f.replace(" ", "_") for f in forms.af.FORMS])
@pytest.mark.parametrize("spec", REL_SPECS, ids=REL_IDS)
def test_every_form_gives_the_canonical_bits_or_a_clear_error(spec, form):
    forms.test_every_form_gives_the_canonical_bits_or_a_clear_error(spec, form)


def rgcn64(layer, rows, col, et, m, x_src, x_dst, p):
    """the layer in fp64 torch, relation by relation: the mean over the neighbours of each (row, relation)"""
    rows, col, et = (torch.from_numpy(np.asarray(a).astype(np.int64)) for a in (rows, col, et))
    out = x_dst @ p["root"] + p["bias"]
    for t in range(layer.num_relations):
        of = et == t
        count = torch.zeros(m, dtype=torch.float64).index_add_(0, rows[of], torch.ones(int(of.sum()), dtype=torch.float64))
        mean = torch.zeros(m, x_src.shape[1], dtype=torch.float64).index_add(0, rows[of], x_src[col[of]]) / count.clamp(min=1)[:, None]
        w = p["weight"][t] if layer.num_bases is None else torch.einsum("b,bio->io", p["comp"][t], p["weight"])
        out = out + mean @ w
    return out


@pytest.mark.parametrize("sampled", [False, True])
@pytest.mark.parametrize("num_bases", [None, 2])
def test_rgcn_conv_matches_the_fp64_per_relation_formulation(num_bases, sampled):
    R, name = 4, "cora" if sampled else "rect"
    rows, col, et, _val, n = entries(name, R, seed=7)
    adj = make_adj(name)
    torch.manual_seed(3)
    layer = gcn_amd.RGCNConv(16, 8, R, num_bases=num_bases).to(DEV)
    x, etd = torch.randn(n, 16), dev(et)
    if sampled:
        (blk,), ids = gcn_amd.sample_blocks(adj, torch.arange(0, n, 5, device=DEV), [4], seed=1)
        adj, x, etd = blk.adj, x[ids.cpu().long()], etd[blk.eid.long()]
        rows, col, et = np.repeat(np.arange(adj.m), np.diff(adj.rowptr.cpu().numpy())), adj.col.cpu().numpy(), etd.cpu().numpy()
    xd = x.to(DEV).requires_grad_(True)
    out = layer(gcn_amd.EdgeTypes(adj, etd, R), (xd, xd[:adj.m]))
    gout = torch.randn(adj.m, 8)
    out.backward(gout.to(DEV))
    p64 = {k: v.detach().cpu().double().requires_grad_(True) for k, v in layer.named_parameters()}
    x64 = x.double().requires_grad_(True)
    ref = rgcn64(layer, rows, col, et, adj.m, x64, x64[:adj.m], p64)
    ref.backward(gout.double())
    pairs = [("out", out, ref), ("grad x", xd.grad, x64.grad)] + [(f"grad {k}", v.grad, p64[k].grad) for k, v in layer.named_parameters()]
    assert len(pairs) == (6 if num_bases else 5)
    for what, got, want in pairs:
        rel = float((got.detach().cpu().double() - want.detach()).abs().max() / want.detach().abs().max())
        print(f"[relational] RGCNConv bases={num_bases} sampled={sampled} {what}: relative error {rel:.2e}")
        assert rel <= 1e-4, (what, rel)


def test_forward_backward_captures_and_replays_bit_for_bit():
    R, B, k = 5, 2, 8
    _rows, _col, et, val, n = entries("boundaries", R, seed=9, masks=True)
    adj = make_adj("boundaries")
    types, vald = gcn_amd.EdgeTypes(adj, dev(et), R), dev(val)
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(n, k, generator=gen).to(DEV).requires_grad_(True)
    coeff = torch.randn(R, B, generator=gen).to(DEV).requires_grad_(True)
    gout = torch.randn(adj.m, B * k, generator=gen).to(DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                      # one eager call: the workspace, the transpose and the relation view exist
        gcn_amd.relation_aggregate(types, x, coeff, vald).backward(gout)
    torch.cuda.current_stream().wait_stream(side)
    x.grad = coeff.grad = None
    graph_ = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph_):
        out = gcn_amd.relation_aggregate(types, x, coeff, vald)
        out.backward(gout)
    for _rep in range(2):
        with torch.no_grad():
            x.copy_(torch.randn(n, k, generator=gen).to(DEV))
            coeff.copy_(torch.randn(R, B, generator=gen).to(DEV))
            gout.copy_(torch.randn(adj.m, B * k, generator=gen).to(DEV))
        graph_.replay()
        torch.cuda.synchronize()
        xe, ce = (t.detach().clone().requires_grad_(True) for t in (x, coeff))
        oe = gcn_amd.relation_aggregate(types, xe, ce, vald)
        oe.backward(gout)
        assert np.array_equal(bits(out), bits(oe)) and np.array_equal(bits(x.grad), bits(xe.grad))
        assert np.array_equal(bits(coeff.grad), bits(ce.grad))

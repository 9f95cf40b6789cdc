"""Grouped matrix product on the GPU (gcn_amd/csrc/segment_mm.hip, gcn_amd.segment_matmul, TypedLinear,
relation_transform_aggregate, RGCNConv(grouped=True)).

References are plain fp64 numpy.  The bound holds for ANY fixed-order fp32 evaluation of a sum of L terms, each term rounded
at most once before it is added: |got - ref| <= (L + 2) 2^-24 sum|terms|, the terms in fp64 from the fp32 inputs (L - 1
additions, the term's rounding, the scale's, one to spare).  The layer is held to the 1e-4 relative of test_relational_gpu.py."""
import importlib

import numpy as np
import pytest
import torch

import gcn_amd
import test_autograd_forms_gpu as forms
from gcn_amd import _lib
from test_aggregate_gpu import bits, make_adj
from test_relational_gpu import dev, entries

_segment_mm = importlib.import_module("gcn_amd.segment_mm")
_relational = importlib.import_module("gcn_amd.relational")
pytestmark = pytest.mark.gpu
WS = importlib.import_module("gcn_amd.spmm").Scratch()           # the workspace of the raw calls below

DEV = "cuda:0"
TM = TN = _lib.SEGMENT_MM_TILE
CHUNK = _lib.SEGMENT_MM_CHUNK
LENS = [0, 1, TM - 1, TM, TM + 1, 0, 2 * TM + 3, 0]
SHAPES = [(1, 1), (3, 5), (32, 32), (33, TN + 1), (68, 2 * TN + 2)]
X_ROWS = 37                                             # rows of a gathered operand: every row is gathered several times


def layout(lens):
    """(segptr int32 [T + 1], N, segment of every row or -1): two uncovered rows in front and two behind"""
    segptr = (2 + np.concatenate([[0], np.cumsum(lens)])).astype(np.int32)
    seg = np.concatenate([[-1, -1], np.repeat(np.arange(len(lens)), lens), [-1, -1]])
    return segptr, len(seg), seg


def case(lens, K, O, gather_x, gather_g, with_scale, seed):
    """fp32 operands of one problem: x, its index or None, g, its index or None, scale or None, W [T, K, O]"""
    rng = np.random.default_rng(seed)
    segptr, N, seg = layout(lens)
    f = lambda *shape: rng.standard_normal(shape).astype(np.float32)
    xi = rng.integers(0, X_ROWS, N).astype(np.int32) if gather_x else None
    gi = rng.integers(0, X_ROWS, N).astype(np.int32) if gather_g else None
    return dict(segptr=segptr, N=N, seg=seg, x=f(X_ROWS if gather_x else N, K), xi=xi, g=f(X_ROWS if gather_g else N, O), gi=gi,
                scale=rng.uniform(0.5, 1.5, N).astype(np.float32) if with_scale else None, W=f(len(lens), K, O))


rows_of = lambda c, a, index: a.astype(np.float64) if index is None else a.astype(np.float64)[index]


def within(got, ref, mag, L, what):
    excess = np.abs(got.detach().cpu().numpy().astype(np.float64) - ref) - ((L + 2) * 2.0 ** -24 * mag + 1e-30)
    print(f"[segment_mm] {what}: max |err| - bound = {excess.max():.3e}")
    assert got.shape == ref.shape and excess.max() <= 0, (what, float(excess.max()))


def ref_forward(c):
    """(y, sum|terms|) fp64 [N, O]; uncovered rows 0"""
    xs, covered = rows_of(c, c["x"], c["xi"]), c["seg"] >= 0
    s = np.ones(c["N"]) if c["scale"] is None else c["scale"].astype(np.float64)
    W = c["W"].astype(np.float64)[np.maximum(c["seg"], 0)]
    y = s[:, None] * np.einsum("ik,iko->io", xs, W) * covered[:, None]
    return y, np.abs(s)[:, None] * np.einsum("ik,iko->io", np.abs(xs), np.abs(W)) * covered[:, None]


def forward(c, transpose_w=False):
    W = c["W"].transpose(0, 2, 1).copy() if transpose_w else c["W"]
    return _segment_mm._forward_raw(WS, dev(c["x"]), dev(c["xi"]), dev(c["scale"]), dev(c["segptr"]), dev(W),
                                    transpose_w, c["N"])


@pytest.mark.parametrize("transpose_w", [False, True])
@pytest.mark.parametrize("with_scale", [False, True])
@pytest.mark.parametrize("gather", [False, True])
@pytest.mark.parametrize("K,O", SHAPES)
def test_forward_matches_fp64_zeroes_uncovered_rows_and_repeats(K, O, gather, with_scale, transpose_w):
    c = case(LENS, K, O, gather, False, with_scale, seed=K + O)
    y = forward(c, transpose_w)
    within(y, *ref_forward(c), K, f"forward K={K} O={O} gather={gather} scale={with_scale} T={transpose_w}")
    assert (y[torch.from_numpy(c["seg"] < 0).to(DEV)] == 0).all()
    assert np.array_equal(bits(forward(c, transpose_w)), bits(y))


@pytest.mark.parametrize("gathers", ["both", "x", "g", "none"])
@pytest.mark.parametrize("K,O", SHAPES)
def test_weight_gradient_matches_fp64_zeroes_empty_segments_and_repeats(K, O, gathers):
    lens = LENS + [2 * CHUNK + 1]
    c = case(lens, K, O, gathers in ("both", "x"), gathers in ("both", "g"), gathers != "x", seed=K + O + 1)
    run = lambda: _segment_mm._wgrad_raw(WS, dev(c["x"]), dev(c["xi"]), dev(c["g"]), dev(c["gi"]), dev(c["scale"]),
                                         dev(c["segptr"]), len(lens), c["N"])
    dw = run()
    xs, gs = rows_of(c, c["x"], c["xi"]), rows_of(c, c["g"], c["gi"])
    if c["scale"] is not None:
        xs = xs * c["scale"].astype(np.float64)[:, None]
    for t, n in enumerate(lens):
        of = c["seg"] == t
        within(dw[t], xs[of].T @ gs[of], np.abs(xs[of]).T @ np.abs(gs[of]), n, f"wgrad K={K} O={O} {gathers} segment {t} ({n} rows)")
        assert n > 0 or (dw[t] == 0).all()
    assert np.array_equal(bits(run()), bits(dw))


def torch64(x, W, c):
    """segment_matmul in fp64 torch: [N, O] (the scale is positive)"""
    seg, s = torch.from_numpy(c["seg"]), torch.from_numpy(c["scale"].astype(np.float64))
    return s[:, None] * torch.einsum("ik,iko->io", x[torch.from_numpy(c["xi"]).long()], W[seg.clamp(min=0)]) * (seg >= 0)[:, None]


def test_autograd_matches_fp64_and_refuses_a_scale_that_requires_grad():
    K, O = 33, TN + 1
    c = case(LENS, K, O, True, False, True, seed=11)
    g = np.random.default_rng(12).standard_normal((c["N"], O)).astype(np.float32)
    x, W = dev(c["x"], grad=True), dev(c["W"], grad=True)
    y = gcn_amd.segment_matmul(x, dev(c["segptr"]), W, index=dev(c["xi"]), scale=dev(c["scale"]))
    within(y, *ref_forward(c), K, "segment_matmul forward")
    y.backward(dev(g))
    res = []
    for xa, Wa, ga in ((c["x"], c["W"], g), (np.abs(c["x"]), np.abs(c["W"]), np.abs(g))):      # the gradients, then sum|terms|
        x64, W64 = (torch.from_numpy(a.astype(np.float64)).requires_grad_(True) for a in (xa, Wa))
        res.append(torch.autograd.grad(torch64(x64, W64, c), (x64, W64), torch.from_numpy(ga.astype(np.float64))))
    (gx, gw), (mx, mw) = res
    within(x.grad, gx.numpy(), mx.numpy(), int(np.bincount(c["xi"]).max()) * O, "segment_matmul grad x")
    within(W.grad, gw.numpy(), mw.numpy(), max(LENS), "segment_matmul grad weight")
    with pytest.raises(ValueError, match="not differentiable"):
        gcn_amd.segment_matmul(x, dev(c["segptr"]), W, index=dev(c["xi"]), scale=dev(c["scale"], grad=True))


@pytest.mark.parametrize("transpose_w", [False, True])
def test_a_nan_row_and_an_inf_weight_stay_where_the_contract_puts_them(transpose_w):
    K, O, nan_row, inf_seg = 33, TN + 1, 5, 4
    c = case(LENS, K, O, True, False, True, seed=21)
    ref, mag = ref_forward(c)
    c["x"][nan_row] = np.nan
    c["W"][inf_seg, 7, 3] = np.inf
    y = forward(c, transpose_w).cpu().numpy()
    gathers_nan, in_inf = (c["xi"] == nan_row) & (c["seg"] >= 0), c["seg"] == inf_seg
    clean = ~gathers_nan & ~in_inf
    assert gathers_nan.sum() > 1 and in_inf.sum() == TM + 1 and clean.sum() > 2 * TM
    assert np.isnan(y[gathers_nan]).all() and not np.isfinite(y[in_inf, 3]).any() and np.isfinite(y[clean]).all()
    within(torch.from_numpy(y[clean]), ref[clean], mag[clean], K, f"the rows beside the non-finite ones T={transpose_w}")


def test_typed_linear_is_the_per_type_product_plus_the_per_type_bias():
    c = case(LENS, 33, TN + 1, False, False, False, seed=31)
    torch.manual_seed(1)
    lin = gcn_amd.TypedLinear(33, TN + 1, len(LENS)).to(DEV)
    out = lin(dev(c["x"]), dev(c["segptr"]))
    out.sum().backward()
    c["W"], covered = lin.weight.detach().cpu().numpy(), c["seg"] >= 0
    bias = lin.bias.detach().cpu().numpy().astype(np.float64)
    ref, mag = ref_forward(c)
    within(out, ref + bias[np.maximum(c["seg"], 0)] * covered[:, None], mag + np.abs(bias[np.maximum(c["seg"], 0)]) * covered[:, None], 33 + 1, "TypedLinear")
    assert np.array_equal(lin.bias.grad.cpu().numpy(), np.repeat(np.array(LENS, np.float32)[:, None], TN + 1, 1))


# ---- the layer ------------------------------------------------------------------------------------------------------------
def rgcn64(rows, col, et, val, m, R, x_src, x_dst, p):
    """RGCNConv without bases in fp64 torch, relation by relation, explicit values"""
    rows, col, et = (torch.from_numpy(np.asarray(a).astype(np.int64)) for a in (rows, col, et))
    val = torch.from_numpy(val.astype(np.float64))
    out = x_dst @ p["root"] + p["bias"]
    for t in range(R):
        of = et == t
        out = out + torch.zeros(m, x_src.shape[1], dtype=torch.float64).index_add(0, rows[of], val[of, None] * x_src[col[of]]) @ p["weight"][t]
    return out


def relative(what, got, want, bound=1e-4):
    rel = float((got.detach().cpu().double() - want.detach().cpu().double()).abs().max() / want.detach().abs().max())
    print(f"[segment_mm] {what}: relative error {rel:.2e}")
    assert got.shape == want.shape and rel <= bound, (what, rel)


@pytest.mark.parametrize("R", [3, 40])
@pytest.mark.parametrize("name", ["boundaries", "rect"])
def test_grouped_rgcn_conv_matches_fp64_and_the_typed_layer(name, R):
    rows, col, et, val, n = entries(name, R, seed=7, masks=True)
    adj = make_adj(name)
    torch.manual_seed(3)
    layer = gcn_amd.RGCNConv(16, 8, R, grouped=True).to(DEV)
    types, x, gout = gcn_amd.EdgeTypes(adj, dev(et), R), torch.randn(n, 16), torch.randn(adj.m, 8)
    xd = x.to(DEV).requires_grad_(True)
    out = layer(types, (xd, xd[:adj.m]), dev(val))
    out.backward(gout.to(DEV))
    p64 = {k: v.detach().cpu().double().requires_grad_(True) for k, v in layer.named_parameters()}
    x64 = x.double().requires_grad_(True)
    ref = rgcn64(rows, col, et, val, adj.m, R, x64, x64[:adj.m], p64)
    ref.backward(gout.double())
    pairs = [("out", out, ref), ("grad x", xd.grad, x64.grad)] + [(f"grad {k}", v.grad, p64[k].grad) for k, v in layer.named_parameters()]
    assert len(pairs) == 5
    for what, got, want in pairs:
        relative(f"grouped RGCNConv {name} R={R} {what}", got, want)
    if R == 3:
        typed = gcn_amd.RGCNConv(16, 8, R).to(DEV)
        typed.load_state_dict(layer.state_dict())
        xt = x.to(DEV).requires_grad_(True)
        out_t = typed(types, (xt, xt[:adj.m]), dev(val))
        out_t.backward(gout.to(DEV))
        for what, got, want in [("out", out, out_t), ("grad x", xd.grad, xt.grad), ("grad weight", layer.weight.grad, typed.weight.grad)]:
            relative(f"grouped against typed {name} {what}", got, want)


def test_grouped_forward_backward_captures_and_replays_bit_for_bit():
    R = 5
    _rows, _col, et, val, n = entries("rect", R, seed=9, masks=True)
    adj = make_adj("rect")
    types, vald = gcn_amd.EdgeTypes(adj, dev(et), R), dev(val)
    torch.manual_seed(4)
    layer = gcn_amd.RGCNConv(12, 7, R, grouped=True).to(DEV)
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(n, 12, generator=gen).to(DEV).requires_grad_(True)
    gout = torch.randn(adj.m, 7, generator=gen).to(DEV)
    step = lambda xx: layer(types, (xx, xx[:adj.m]), vald)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                      # one eager call: the workspaces, the transpose and the relation view exist
        step(x).backward(gout)
    torch.cuda.current_stream().wait_stream(side)
    x.grad = None
    layer.zero_grad(set_to_none=True)
    graph_ = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph_):
        out = step(x)
        out.backward(gout)
    with torch.no_grad():
        x.copy_(torch.randn(n, 12, generator=gen).to(DEV)), gout.copy_(torch.randn(adj.m, 7, generator=gen).to(DEV))
    graph_.replay()
    torch.cuda.synchronize()
    captured = [bits(t) for t in (out, x.grad, layer.weight.grad, layer.root.grad, layer.bias.grad)]
    layer.zero_grad(set_to_none=True)
    xe = x.detach().clone().requires_grad_(True)
    oe = step(xe)
    oe.backward(gout)
    for got, want in zip(captured, (oe, xe.grad, layer.weight.grad, layer.root.grad, layer.bias.grad)):
        assert np.array_equal(got, bits(want))


# ---- the autograd contract (tests/autograd_forms.py) on the two new Functions: entered into the SPECS of
# tests/test_autograd_forms_gpu.py on import, as test_relational_gpu.py does; small integers, so fp64 gives the same bits
def segment_specs():
    c = case(LENS, 5, 6, True, False, True, seed=41)
    scale = np.round(c["scale"]).astype(np.float32) + 1                        # 1 or 2 or 3
    seg, xi = c["seg"], c["xi"]

    def make(seed, device):
        return [forms.ints((X_ROWS, 5), 70 * seed, 4, device), forms.ints((len(LENS), 5, 6), 70 * seed + 1, 2, device)], \
            forms.ints((c["N"], 6), 70 * seed + 2, 4, device)

    def reference(x, w):
        t, s = torch.from_numpy(seg).to(x.device), torch.from_numpy(scale).to(device=x.device, dtype=x.dtype)
        y = s[:, None] * torch.einsum("ik,iko->io", x[torch.from_numpy(xi).long().to(x.device)], w[t.clamp(min=0)])
        return y * (t >= 0)[:, None]

    def build():
        gather, segptr, s = gcn_amd.RowGather(dev(xi), X_ROWS), dev(c["segptr"]), dev(scale)
        return (lambda x, w: gcn_amd.segment_matmul(x, segptr, w, index=gather, scale=s)), None
    specs = [forms.Spec("segment_matmul gathered scaled", [_segment_mm._SegmentMatmulFunction], make, reference, build)]

    P, R = forms.pattern("rect"), 4
    rng = np.random.default_rng(R)
    et, val = rng.integers(-1, R + 1, P.nnz), rng.integers(1, 3, P.nnz).astype(np.float32)
    keep = np.flatnonzero((et >= 0) & (et < R))

    def make_r(seed, device):
        return [forms.ints((P.n, 5), 80 * seed, 4, device), forms.ints((R, 5, 3), 80 * seed + 1, 2, device)], \
            forms.ints((P.m, 3), 80 * seed + 2, 4, device)

    def reference_r(x, w):
        row, col = (t[torch.from_numpy(keep).to(x.device)] for t in P.index(x.device))
        t, v = torch.from_numpy(et[keep]).to(x.device), torch.from_numpy(val[keep]).to(device=x.device, dtype=x.dtype)
        return torch.zeros(P.m, w.shape[2], dtype=x.dtype, device=x.device).index_add(
            0, row, v[:, None] * torch.einsum("ek,eko->eo", x[col], w[t]))

    def build_r():
        types, v = gcn_amd.EdgeTypes(P.adj("relation_transform"), dev(et.astype(np.int32)), R), dev(val)
        return (lambda x, w: gcn_amd.relation_transform_aggregate(types, x, w, v)), None
    return specs + [forms.Spec("relation_transform_aggregate R=4", [_relational._RelationTransformFunction], make_r, reference_r, build_r)]


SEG_SPECS = segment_specs()
SEG_IDS = [s.name.replace(" ", "_") for s in SEG_SPECS]
if not any(s.name == SEG_SPECS[0].name for s in forms.SPECS):
    forms.SPECS = forms.SPECS + SEG_SPECS


@pytest.mark.parametrize("spec", SEG_SPECS, ids=SEG_IDS)
def test_the_canonical_call_matches_fp64_autograd_of_the_plain_formulation(spec):
    forms.test_the_canonical_call_matches_fp64_autograd_of_the_plain_formulation(spec)


@pytest.mark.parametrize("form", list(forms.af.FORMS), ids=[f.replace(" ", "_") for f in forms.af.FORMS])
@pytest.mark.parametrize("spec", SEG_SPECS, ids=SEG_IDS)
def test_every_form_gives_the_canonical_bits_or_a_clear_error(spec, form):
    forms.test_every_form_gives_the_canonical_bits_or_a_clear_error(spec, form)

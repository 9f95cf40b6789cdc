"""The autograd contract of every torch.autograd.Function of gcn_amd on the GPU ("The autograd contract"): each
op's canonical call is anchored once against fp64 torch autograd of its plain formulation, then every form of
tests/autograd_forms.py — frozen operands, strided operands and gradients, repeated and shared use, later calls, in-place
changes, changed adjacency values, no_grad, second differentiation — must give the canonical bits or a clear error.

Patterns: `rect` (60 x 300, rows on either side of every threshold of the long-row kernels, a column of more than 4096
entries so that the transposed walks have a chunked row too) and `square` (cora).  The non-softmax ops run on the exact grids
of their own test files (integers / eighths: any correct summation order gives the same bits), the softmax ops on standard
normal inputs within the bounds of test_heads_gpu.py.  Also here: the two GATv2 backward combinations no wrapper reaches,
through the C ABI, and the layers with each parameter frozen in turn."""
import functools
import importlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F_

import autograd_forms as af
import gatv2_ref
import gcn_amd
import heads_ref
import util
from gcn_amd import graphgen

# (the modules, not the functions of the same names that the package exports)
_aggregate, _attention, _layers, _spgemm, _spmm = (importlib.import_module("gcn_amd." + name)
                                                   for name in ("aggregate", "attention", "layers", "spgemm", "spmm"))

DEV = "cuda:0"
RECT_LENS = [0, 0, 1, 2, 63, 64, 65, 257, 4097, 8193]
F32, BF16 = torch.float32, torch.bfloat16


# ---- patterns -------------------------------------------------------------------------------------------------------------------
class Pattern:
    def __init__(self, rowptr, col, n):
        self.rowptr, self.col, self.n = np.asarray(rowptr, np.int32), np.asarray(col, np.int32), int(n)
        self.m, self.nnz = len(self.rowptr) - 1, len(self.col)
        self.lens = np.diff(self.rowptr.astype(np.int64))
        self.row = heads_ref.entry_rows(self.rowptr)
        self._index, self._adj = {}, {}

    def index(self, device):
        """(row, col) of every entry as int64 tensors"""
        device = str(device)
        if device not in self._index:
            self._index[device] = (torch.from_numpy(self.row).to(device), torch.from_numpy(self.col.astype(np.int64)).to(device))
        return self._index[device]

    def values(self):
        return util.int_values(self.nnz, 77)

    def adj(self, key, mutable=False):
        """a device adjacency on this pattern with integer values; one per key"""
        if key not in self._adj:
            self._adj[key] = gcn_amd.CsrAdjacency(torch.from_numpy(self.rowptr).to(DEV), torch.from_numpy(self.col).to(DEV),
                                                  torch.from_numpy(self.values()).to(DEV), (self.m, self.n), symmetric=False,
                                                  mutable_values=mutable)
        return self._adj[key]


@functools.lru_cache(maxsize=None)
def pattern(name):
    if name == "rect":
        rng = np.random.default_rng(2024)
        lens = np.concatenate([RECT_LENS, rng.poisson(12, 40), np.zeros(10, np.int64)]).astype(np.int64)
        rows = np.repeat(np.arange(len(lens)), lens)
        cols = rng.integers(0, 300, len(rows))
        cols[rng.random(len(rows)) < 0.35] = 3
        order = np.lexsort((cols, rows))
        p = Pattern(np.concatenate([[0], np.cumsum(lens)]), cols[order], 300)
        assert int((p.col == 3).sum()) > 4096 and p.nnz < 16000        # a chunked row of the transposed pattern; small
        return p
    rp, col, _v, n = graphgen.make_graph("cora", device="cpu", seed=1)
    return Pattern(rp.numpy(), col.numpy(), n)


def ints(shape, seed, top, device, dtype=F32, scale=1.0):
    a = np.random.default_rng(seed).integers(-top, top + 1, shape).astype(np.float32) * scale
    return torch.from_numpy(a).to(device=device, dtype=dtype)


def normal(shape, seed, device):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(device)


# ---- specs ----------------------------------------------------------------------------------------------------------------------
class Spec:
    """one op of the sweep: make(seed, device) -> (operands, g); reference(*operands) the plain formulation (any dtype, any
    device); build() -> (call, mutate) on the GPU; functions: the autograd Functions its call goes through"""

    def __init__(self, name, functions, make, reference, build, grid=True, share=None, anchor=None, out_dtype=None):
        self.name, self.functions, self.make, self.reference, self.build = name, functions, make, reference, build
        self.grid, self.share, self.anchor, self.out_dtype = grid, share, anchor, out_dtype
        self._op = None

    def op(self):
        if self._op is None:
            call, mutate = self.build()
            self._op = af.Op(self.name, lambda seed: self.make(seed, DEV), call, mutate=mutate, share=self.share)
        return self._op


def fp64_reference(spec, operands, g):
    leaves = [t.detach().double().requires_grad_(True) for t in operands]
    out = spec.reference(*leaves)
    grads = torch.autograd.grad(out, leaves, g.double(), allow_unused=False)
    return out.detach(), {i: gr for i, gr in enumerate(grads)}


SPECS = []


def mutate_of(adj):
    def mutate():
        old = adj.val.clone()
        adj.update_values(-old - 1)
        return lambda: adj.update_values(old)
    return mutate


def ref_spmm(P, x, v):
    row, col = P.index(x.device)
    return torch.zeros(P.m, x.shape[1], dtype=x.dtype, device=x.device).index_add(0, row, v[:, None] * x[col])


def add_spmm():
    P = pattern("rect")
    for dtype, mutable, k in ((F32, False, 8), (F32, True, 40), (BF16, False, 40), (BF16, True, 8)):
        name = f"spmm {'bf16' if dtype == BF16 else 'fp32'} {'mutable' if mutable else 'fixed'} k={k}"

        def make(seed, device, k=k, dtype=dtype):
            return [ints((P.n, k), 10 * seed + k, 8, device, dtype)], ints((P.m, k), 10 * seed + k + 1, 8, device, dtype)

        def reference(x):
            return ref_spmm(P, x, torch.from_numpy(P.values()).to(x.device, x.dtype))

        def build(name=name, mutable=mutable):
            adj = P.adj(name, mutable)
            return (lambda x: gcn_amd.spmm(adj, x)), (mutate_of(adj) if mutable else None)
        SPECS.append(Spec(name, [_spmm._SpmmFunction], make, reference, build, out_dtype=dtype))
    for k in (8, 40):
        def make(seed, device, k=k):
            v = torch.from_numpy(util.int_values(P.nnz, 300 + seed)).to(device)
            return [ints((P.n, k), 20 * seed + k, 8, device), v], ints((P.m, k), 20 * seed + k + 1, 8, device)

        def build(k=k):
            adj = P.adj(f"values {k}", True)
            return (lambda x, v: gcn_amd.spmm(adj, x, values=v)), None
        SPECS.append(Spec(f"spmm values k={k}", [_spmm._SpmmValuesFunction], make, lambda x, v: ref_spmm(P, x, v), build))
    S = pattern("square")

    def make(seed, device):
        v = torch.from_numpy(util.int_values(S.nnz, 400 + seed)).to(device)
        return [v, ints((S.n, 8), 30 + seed, 8, device)], ints((S.m, 8), 40 + seed, 8, device)

    def build():
        row, col = S.index(DEV)
        idx = torch.stack([row, col])

        def call(v, b):
            gcn_amd.install(sparse_grad=True)              # (idempotent; every test of this file uninstalls in a finally)
            return torch.sparse.mm(torch.sparse_coo_tensor(idx, v, (S.m, S.n), is_coalesced=True), b)
        return call, None
    SPECS.append(Spec("torch.sparse.mm routed, k=8", [_spmm._SparseMmGrad], make, lambda v, b: ref_spmm(S, b, v), build))


def add_fused():
    p, seed_, offset = util.EPILOGUE_DROPOUT
    for pname, k, drop, mutable, through_layer in (("square", 8, None, False, True), ("square", 40, (p, seed_, offset), True, True),
                                                   ("rect", 8, (p, seed_, offset), True, False)):
        P = pattern(pname)
        name = f"fused epilogue {pname} k={k} dropout={drop[0] if drop else 0} {'layer' if through_layer else 'direct'}"

        def make(seed, device, P=P, k=k):
            return [ints((P.n, k), 50 * seed + k, 8, device), ints((k,), 50 * seed + k + 1, 8, device)], ints((P.m, k), 50 * seed + k + 2, 8, device)

        def reference(x, bias, P=P, k=k, drop=drop):
            z = torch.relu(ref_spmm(P, x, torch.from_numpy(P.values()).to(x.device, x.dtype)) + bias)
            if drop is None:
                return z
            keep = torch.from_numpy(util.dropout_keep(P.m * k, *drop).reshape(P.m, k)).to(x.device)
            return z * keep * (1.0 / (1.0 - drop[0]))

        def build(P=P, k=k, drop=drop, mutable=mutable, through_layer=through_layer, name=name):
            adj = P.adj(name, mutable)
            if not through_layer:
                return (lambda x, b: _layers._FusedSpmmBiasRelu.apply(adj, x, b, True, drop)), (mutate_of(adj) if mutable else None)
            layer = gcn_amd.GraphConvolution(k, k).to(DEV)
            eye = torch.eye(k, device=DEV)                 # (X·W with W = I: the layer's own matmul, exact)

            def call(x, b):
                return torch.func.functional_call(layer, {"weight": eye, "bias": b}, (x, adj),
                                                  dict(relu=True, fuse_epilogue=True, dropout=drop))
            return call, (mutate_of(adj) if mutable else None)
        SPECS.append(Spec(name, [_layers._FusedSpmmBiasRelu], make, reference, build))


def ref_select(P, x, reduce):
    """row-wise max / min with the kernel's tie rule — the lowest entry index — so that the gradient goes to that entry"""
    row, col = P.index(x.device)
    k = x.shape[1]
    E = x[col]
    key = -E.detach() if reduce == "min" else E.detach()
    ridx = row[:, None].expand(-1, k).contiguous()
    best = torch.full((P.m, k), float("-inf"), dtype=x.dtype, device=x.device).scatter_reduce(0, ridx, key, "amax")
    eidx = torch.arange(P.nnz, device=x.device)[:, None].expand(-1, k).contiguous()
    cand = torch.where(key == best[row], eidx, P.nnz)
    arg = torch.full((P.m, k), P.nnz, dtype=torch.int64, device=x.device).scatter_reduce(0, ridx, cand, "amin")
    picked = E[arg.clamp(max=P.nnz - 1), torch.arange(k, device=x.device)[None, :]]
    return torch.where(arg < P.nnz, picked, torch.zeros_like(picked))


def add_aggregate():
    P = pattern("rect")
    cases = [("max", F32, 5, False), ("max", BF16, 64, False), ("min", F32, 64, False), ("min", BF16, 5, False),
             ("sum", F32, 5, False), ("mean", F32, 64, False), ("sum", F32, 64, True), ("mean", F32, 5, True)]
    for reduce, dtype, k, mutable in cases:
        name = f"aggregate {reduce} {'bf16' if dtype == BF16 else 'fp32'} k={k}{' mutable' if mutable else ''}"

        def make(seed, device, k=k, dtype=dtype):
            return [ints((P.n, k), 60 * seed + k, 8, device, dtype)], ints((P.m, k), 60 * seed + k + 1, 8, device, dtype)

        def reference(x, reduce=reduce):
            if reduce in ("max", "min"):
                return ref_select(P, x, reduce)
            w = torch.ones(P.nnz, dtype=x.dtype, device=x.device)
            if reduce == "mean":
                w = w / torch.from_numpy(np.maximum(P.lens, 1)[P.row]).to(x.device, x.dtype)
            return ref_spmm(P, x, w)

        def build(name=name, reduce=reduce, mutable=mutable):
            adj = P.adj(name, mutable)
            return (lambda x: gcn_amd.aggregate(adj, x, reduce)), (mutate_of(adj) if mutable else None)
        fn = _aggregate._SelectFunction if reduce in ("max", "min") else _spmm._SpmmFunction
        # mean: the values 1 / row length are not on the grid; its canonical call is held to the standing bound instead
        SPECS.append(Spec(name, [fn], make, reference, build, grid=reduce != "mean", anchor=anchor_mean if reduce == "mean" else None,
                          out_dtype=dtype))


def anchor_mean(spec):
    operands, g, out, grads = af.canonical(spec.op())
    ref_out, ref_grads = fp64_reference(spec, operands, g)
    mag_out, mag_grads = fp64_reference(spec, [operands[0].abs()], g.abs())
    for what, got, ref, mag in (("output", out, ref_out, mag_out), ("gradient", grads[0], ref_grads[0], mag_grads[0])):
        ratio = float(((got.double() - ref).abs() / (1e-5 * mag + 1e-30)).max())
        print(f"[forms] {spec.name} {what}: max error / bound = {ratio:.4f}")
        assert ratio <= 1.0, (spec.name, what, ratio)


# ---- the softmax ops: standard normal inputs, the bounds of test_heads_gpu.py ---------------------------------------------------
def heads_graph(P):
    import test_heads_gpu
    return test_heads_gpu.Graph(P.rowptr, P.col, P.n), test_heads_gpu


def anchor_edge_softmax(spec):
    P = pattern("rect")
    hg, th = heads_graph(P)
    operands, g, out, grads = af.canonical(spec.op())
    two = (lambda t: t.cpu().numpy().reshape(P.nnz, -1))
    s, p, gn, ds = two(operands[0]), two(out), two(g), two(grads[0])
    H = s.shape[1]
    th.check_forward(hg, H, s, p, spec.name)
    ratio = float((np.abs(ds - heads_ref.edge_softmax_backward(P.rowptr, p, gn)) / th.ds_bound(hg, H, p, gn)).max())
    print(f"[forms] {spec.name} backward: max error / bound = {ratio:.4f}")
    assert ratio <= 1.0, (spec.name, ratio)


def anchor_gat_edge_softmax(spec, slope):
    P = pattern("rect")
    hg, th = heads_graph(P)
    operands, g, out, grads = af.canonical(spec.op())
    ad, asrc = operands[0].cpu().numpy().reshape(P.m, -1), operands[1].cpu().numpy().reshape(P.n, -1)
    p, gn = out.cpu().numpy().reshape(P.nnz, -1), g.cpu().numpy().reshape(P.nnz, -1)
    H = p.shape[1]
    th.check_forward(hg, H, heads_ref.gat_scores(P.rowptr, P.col, ad, asrc, slope), p, spec.name)
    ds_ref, gd_ref = heads_ref.gat_edge_softmax_backward(P.rowptr, P.col, ad, asrc, slope, p, gn)
    trp, _trow, tperm = heads_ref.transpose_pattern(P.rowptr, P.col, P.n)
    for what, got, ref, mag in (("grad_a_dst", grads[0], gd_ref, heads_ref.row_sums(P.rowptr, np.abs(ds_ref))),
                                ("grad_a_src", grads[1], heads_ref.segment_sum(trp, ds_ref, tperm),
                                 heads_ref.segment_sum(trp, np.abs(ds_ref), tperm))):
        ratio = float((np.abs(got.cpu().numpy().reshape(ref.shape) - ref) / (1e-5 * mag + 1e-30)).max())
        print(f"[forms] {spec.name} {what}: max error / bound = {ratio:.4f}")
        assert ratio <= 1.0, (spec.name, what, ratio)


def add_softmax():
    P = pattern("rect")
    for H in (None, 4, 3):
        tail = () if H is None else (H,)

        def make(seed, device, tail=tail):
            return [normal((P.nnz,) + tail, 70 + seed, device)], normal((P.nnz,) + tail, 80 + seed, device)

        def build(H=H):
            adj = P.adj("softmax")
            return (lambda s: gcn_amd.edge_softmax(adj, s)), None
        SPECS.append(Spec(f"edge_softmax {'1-D' if H is None else f'H={H}'}", [_attention._EdgeSoftmaxFunction], make, None, build,
                          grid=False, anchor=anchor_edge_softmax))
    for H, slope in ((None, 0.2), (4, 0.2), (3, 1.5)):
        tail = () if H is None else (H,)

        def make(seed, device, tail=tail):
            return ([normal((P.m,) + tail, 90 + seed, device), normal((P.n,) + tail, 95 + seed, device)],
                    normal((P.nnz,) + tail, 99 + seed, device))

        def build(H=H, slope=slope):
            adj = P.adj("gat softmax", mutable=True) if H is None else P.adj("softmax")
            return (lambda d, s: gcn_amd.gat_edge_softmax(adj, d, s, slope)), None
        SPECS.append(Spec(f"gat_edge_softmax {'1-D mutable' if H is None else f'H={H}'} slope={slope}",
                          [_attention._GatEdgeSoftmaxFunction], make, None, build, grid=False,
                          anchor=functools.partial(anchor_gat_edge_softmax, slope=slope)))


# ---- the head-batched gathers and the GATv2 scores, on their grids ----------------------------------------------------------------
def ref_spmm_heads(P, x, v):
    row, col = P.index(x.device)
    H = v.shape[1]
    t = v[:, :, None] * x[col].view(P.nnz, H, -1)
    return torch.zeros((P.m,) + tuple(t.shape[1:]), dtype=x.dtype, device=x.device).index_add(0, row, t).view(P.m, -1)


def ref_sddmm_heads(P, a, b, H):
    row, col = P.index(a.device)
    return (a[row].view(P.nnz, H, -1) * b[col].view(P.nnz, H, -1)).sum(-1)


def ref_gatv2(P, hd, hs, att, slope):
    row, col = P.index(hd.device)
    return (F_.leaky_relu(hd[row] + hs[col], slope).view(P.nnz, att.shape[0], att.shape[1]) * att).sum(-1)


def add_heads():
    R, S = pattern("rect"), pattern("square")
    for H, F in ((4, 8), (3, 5)):
        def make(seed, device, H=H, F=F):
            return ([ints((R.n, H * F), 110 * seed + F, 3, device), ints((R.nnz, H), 110 * seed + F + 1, 7, device, scale=0.125).abs()],
                    ints((R.m, H * F), 110 * seed + F + 2, 3, device))
        SPECS.append(Spec(f"spmm_heads {H}x{F}", [_attention._SpmmHeadsFunction], make, lambda x, v: ref_spmm_heads(R, x, v),
                          lambda: ((lambda x, v: gcn_amd.spmm_heads(R.adj("heads"), x, v)), None)))
    for P, H, F, share in ((R, 4, 8, None), (R, 3, 5, None), (S, 4, 8, (0, 1))):
        def make(seed, device, P=P, H=H, F=F):
            return ([ints((P.m, H * F), 120 * seed + F, 3, device), ints((P.n, H * F), 120 * seed + F + 1, 3, device)],
                    ints((P.nnz, H), 120 * seed + F + 2, 7, device, scale=0.125))
        SPECS.append(Spec(f"sddmm_heads {H}x{F}{' square' if share else ''}", [_attention._SddmmHeadsFunction], make,
                          lambda a, b, P=P, H=H: ref_sddmm_heads(P, a, b, H),
                          lambda P=P, H=H: ((lambda a, b: gcn_amd.sddmm_heads(P.adj("heads"), a, b, H)), None), share=share))
    for P, H, F, share in ((R, 4, 8, None), (R, 3, 5, None), (R, 8, 40, None), (S, 4, 8, (0, 1))):
        def make(seed, device, P=P, H=H, F=F):
            return ([ints((P.m, H * F), 130 * seed + F, 2, device), ints((P.n, H * F), 130 * seed + F + 1, 2, device),
                     ints((H, F), 130 * seed + F + 2, 2, device)], ints((P.nnz, H), 130 * seed + F + 3, 7, device, scale=0.125))
        SPECS.append(Spec(f"gatv2_scores {H}x{F}{' square' if share else ''}", [_attention._Gatv2ScoresFunction], make,
                          lambda hd, hs, att, P=P: ref_gatv2(P, hd, hs, att, 0.5),
                          lambda P=P: ((lambda hd, hs, att: gcn_amd.gatv2_scores(P.adj("heads"), hd, hs, att, 0.5)), None), share=share))


# ---- the sparse product and the hypergraph Laplacian ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def product_pair():
    """the 300 x 200 · 200 x 400 pair of test_sparse_product_gpu.py (repeats in A, B ascending) and the pattern of C"""
    import scipy.sparse as sp
    from test_sampled_dot_cpu import _sorted
    from test_spgemm_cpu import _random_csr
    rng = np.random.default_rng(21)
    a = _random_csr(300, 200, 0.05, rng, repeats=True)
    b = _sorted(*_random_csr(200, 400, 0.05, rng))
    ones = lambda x, shape: sp.csr_matrix((np.ones(len(x[1])), x[1], x[0]), shape=shape)
    c = (ones(a, (300, 200)) @ ones(b, (200, 400))).tocsr()
    c.sort_indices()
    return a, b, Pattern(c.indptr, c.indices, 400)


@functools.lru_cache(maxsize=None)
def product_on_device():
    a, b, C = product_pair()
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    A = gcn_amd.CsrAdjacency(t(a[0]), t(a[1]), t(a[2]), (300, 200), chunk_nnz=4096)
    B = gcn_amd.CsrAdjacency(t(b[0]), t(b[1]), t(b[2]), (200, 400))
    prod = gcn_amd.SparseProduct(A, B)
    assert prod.adj.nnz == C.nnz and torch.equal(prod.adj.rowptr.cpu(), torch.from_numpy(C.rowptr))
    return prod


def add_products():
    a, b, C = product_pair()
    A_, B_ = Pattern(a[0], a[1], 200), Pattern(b[0], b[1], 400)

    def make(seed, device):
        return ([torch.from_numpy(util.int_values(A_.nnz, 500 + seed)).to(device), torch.from_numpy(util.int_values(B_.nnz, 510 + seed)).to(device)],
                ints((C.nnz,), 520 + seed, 8, device))

    def reference(av, bv):
        dense = lambda P, v: torch.zeros(P.m, P.n, dtype=v.dtype, device=v.device).index_put(P.index(v.device), v, accumulate=True)
        if av.is_cuda:                                     # (the entry order of the product's own pattern)
            adj = product_on_device().adj
            crow = torch.repeat_interleave(torch.arange(adj.m, device=av.device), (adj.rowptr[1:] - adj.rowptr[:-1]).long())
            ccol = adj.col.long()
        else:
            crow, ccol = C.index(av.device)
        return (dense(A_, av) @ dense(B_, bv))[crow, ccol]
    SPECS.append(Spec("SparseProduct.values", [_spgemm._SparseProductFunction], make, reference,
                      lambda: ((lambda av, bv: product_on_device().values(av, bv)), None)))

    def make_w(seed, device):
        rng = np.random.default_rng(600 + seed)
        w = torch.from_numpy((0.25 + rng.random(12)).astype(np.float32)).to(device)
        return [w], normal((laplacian().adj.nnz,), 610 + seed, device)
    SPECS.append(Spec("HypergraphLaplacian.values", [_spgemm._LaplacianFunction], make_w, None,
                      lambda: ((lambda w: laplacian().values(w)), None), grid=False, anchor=anchor_laplacian))


@functools.lru_cache(maxsize=None)
def laplacian():
    import test_hgnn_gpu
    H, _dense, _w = test_hgnn_gpu.fixture_h()
    return gcn_amd.HypergraphLaplacian(H)


def anchor_laplacian(spec):
    """the two criteria of test_hgnn_gpu.py: the values are hypergraph_laplacian's bit for bit, the gradient lies within
    4 x the error the dense formula makes when differentiated in fp32"""
    import test_hgnn_gpu as th
    H, dense, _w = th.fixture_h()
    L = laplacian()
    operands, g, out, grads = af.canonical(spec.op())
    assert th.same_bits(out, gcn_amd.hypergraph_laplacian(H, operands[0]).val)
    Cd = th.dense_of(L.adj, g)
    res = {}
    for dtype in (torch.float64, torch.float32):
        wd = operands[0].clone().to(dtype).requires_grad_(True)    # (a copy: the canonical operands are left alone)
        Gd = th.dense_g_torch(th.t(dense).to(dtype), wd)
        (gr,) = torch.autograd.grad((Gd * Cd.to(dtype)).sum(), wd)
        res[dtype] = (Gd.detach(), gr)
    for what, got, r64, r32 in (("gradient", grads[0], res[torch.float64][1], res[torch.float32][1]),):
        ours, dense32 = float((got.double() - r64).abs().max()), float((r32.double() - r64).abs().max())
        print(f"[forms] {spec.name} {what}: |ours - fp64| = {ours:.3e}, |dense fp32 - fp64| = {dense32:.3e}")
        assert dense32 > 0 and ours <= 4 * dense32, (what, ours, dense32)


add_spmm()
add_fused()
add_aggregate()
add_softmax()
add_heads()
add_products()
SPEC_IDS = [s.name.replace(" ", "_") for s in SPECS]
assert len(set(SPEC_IDS)) == len(SPECS)


# ---- the tests ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("spec", SPECS, ids=SPEC_IDS)
def test_the_canonical_call_matches_fp64_autograd_of_the_plain_formulation(spec):
    try:
        if spec.anchor is not None:
            return spec.anchor(spec)
        operands, g, out, grads = af.canonical(spec.op())
        ref_out, ref_grads = fp64_reference(spec, operands, g)
        for what, got, ref in [("output", out, ref_out)] + [(f"gradient {i}", grads[i], ref_grads[i]) for i in grads]:
            assert torch.equal(ref.float().double(), ref), f"{spec.name}: the fp64 {what} is not on the fp32 grid"
            assert got.shape == ref.shape and torch.equal(got, ref.float().to(got.dtype)), f"{spec.name}: {what} differs from fp64"
    finally:
        gcn_amd.uninstall()


@pytest.mark.gpu
@pytest.mark.parametrize("form", list(af.FORMS), ids=[f.replace(" ", "_") for f in af.FORMS])
@pytest.mark.parametrize("spec", SPECS, ids=SPEC_IDS)
def test_every_form_gives_the_canonical_bits_or_a_clear_error(spec, form):
    try:
        af.FORMS[form](spec.op())
    finally:
        gcn_amd.uninstall()


# ---- the GATv2 backward through the C ABI: the two combinations the wrapper cannot reach or no test reaches ----------------------
@pytest.mark.gpu
@pytest.mark.parametrize("by", [0, 1])
@pytest.mark.parametrize("H,F", [(4, 8), (3, 5), (8, 40)])
def test_gatv2_backward_pattern_walk_without_act_sums_and_transposed_walk_with_them(H, F, by):
    import test_gatv2_gpu as tg
    P = pattern("rect")
    g = tg.Graph(P.rowptr, P.col, P.n)
    c = tg.Case(g, H, F, 0.5, seed=1000 + 10 * H + F, grid=True)
    trp, trow, tperm = g.t
    # the transposed walk's own sums: the twin on the transposed pattern, the two sides exchanged
    gs_t, _gd_t, act_t, _ga = gatv2_ref.backward(trp, trow, g.m, c.hs, c.hd, c.att, c.slope, c.g[tperm])
    assert np.array_equal(gs_t, c.gs)
    raw = tg.Raw(g, by)
    k = c.k
    hd, hs, att, gg = raw.put(c.hd), raw.put(c.hs), raw.put(c.att), raw.put(c.g)
    ws = raw.ws(H, k)
    outs = [raw.out(g.m, k), raw.out(g.n, k), raw.out(g.n, k)]
    (gd, _), (gs, _), (act, _) = outs
    vp, lib = tg.vp, raw.lib
    st = [lib.gcn_gatv2_scores_backward_csr_f32(vp(raw.rowptr), vp(raw.col), None, g.m, g.nnz, H, k, vp(hd), vp(hs), vp(att), c.slope,
                                                vp(gg), vp(gd), None, vp(ws), ws.numel(), tg.stream()),
          lib.gcn_gatv2_scores_backward_csr_f32(vp(raw.trp), vp(raw.trow), vp(raw.tperm), g.n, g.nnz, H, k, vp(hs), vp(hd), vp(att),
                                                c.slope, vp(gg), vp(gs), vp(act), vp(ws), ws.numel(), tg.stream())]
    torch.cuda.synchronize()
    assert st == [0, 0], st
    for view, flat in outs + raw.held:
        assert util.guards_intact(flat, view), "a call wrote outside its arrays"
    what = f"{H}x{F} shifted by {by}"
    assert torch.equal(gd, tg.dev(tg.on_grid(c.gd))), what + ": grad_h_dst of the pattern walk without act_sums"
    assert torch.equal(gs, tg.dev(tg.on_grid(c.gs))), what + ": grad_h_src of the transposed walk with act_sums"
    assert torch.equal(act, tg.dev(tg.on_grid(act_t))), what + ": act_sums of the transposed walk"


# ---- layers with each parameter frozen in turn ----------------------------------------------------------------------------------
def _frozen_parameter_check(make_layer, run):
    """for each parameter in turn: frozen, the gradients of the others are the bits of the all-trainable run on the same
    weights, and it keeps .grad None"""
    torch.manual_seed(17)
    layer = make_layer().to(DEV)
    with torch.no_grad():
        for p in layer.parameters():
            if float(p.abs().max()) == 0.0:                # (a bias initialised to zeros)
                p.normal_()
    out = run(layer)
    gout = normal(tuple(out.shape), 18, DEV)
    out.backward(gout)
    want = {k: p.grad.clone() for k, p in layer.named_parameters()}
    assert len(want) >= 2 and all(bool(v.abs().max() > 0) for v in want.values())
    for frozen, _p in layer.named_parameters():
        layer.zero_grad(set_to_none=True)
        for k, p in layer.named_parameters():
            p.requires_grad_(k != frozen)
        got = run(layer)
        assert torch.equal(got.detach(), out.detach()), frozen
        got.backward(gout)
        for k, p in layer.named_parameters():
            if k == frozen:
                assert p.grad is None, f"{frozen} is frozen and got a gradient"
            else:
                assert p.grad is not None and torch.equal(p.grad, want[k]), f"{frozen} frozen: the gradient of {k} changed"


def _square_x(width):
    return normal((pattern("square").n, width), 19, DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("head_batched", [False, True])
def test_graph_attention_with_each_parameter_frozen(head_batched):
    S = pattern("square")
    adj, x = S.adj("gat layer", mutable=True), _square_x(24)
    _frozen_parameter_check(lambda: gcn_amd.GraphAttention(24, 8, heads=4, head_batched=head_batched), lambda layer: layer(x, adj))


@pytest.mark.gpu
@pytest.mark.parametrize("share", [False, True])
def test_graph_attention_v2_with_each_parameter_frozen(share):
    S = pattern("square")
    adj, x = S.adj("heads"), _square_x(24)
    _frozen_parameter_check(lambda: gcn_amd.GraphAttentionV2(24, 8, heads=4, share_weights=share), lambda layer: layer(x, adj))


@pytest.mark.gpu
def test_sage_conv_max_with_each_parameter_frozen():
    S = pattern("square")
    adj, x = S.adj("heads"), _square_x(24)
    _frozen_parameter_check(lambda: gcn_amd.SAGEConv(24, 8, aggr="max"), lambda layer: layer(x, adj))


@pytest.mark.gpu
def test_hgnn_conv_with_each_parameter_frozen():
    S = pattern("square")
    adj, x = S.adj("hgnn layer"), _square_x(24)
    _frozen_parameter_check(lambda: gcn_amd.HGNNConv(24, 8), lambda layer: layer(x, adj))

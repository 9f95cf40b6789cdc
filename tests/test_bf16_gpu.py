"""bf16 feature operands (gcn_spmm_csr_bf16_epilogue, spmm_group_bf16.hip) on the GPU: the hot path (bf16 group walk,
value-free and weighted), the fallback (widen, fp32 entry, narrow) on every other plan and width, the epilogue and its
dropout mask, determinism, autograd, bf16 training of the GCN, and the headline graph once at full size.

Error bound (elementwise, against the fp64 oracle on the upcast inputs):
    |C - C*| <= 2^-8 * (|A|.|B|) + 2^-8 * |C*| + 1e-6
the first term for the rounded value-free table, the second for the bf16 rounding of the result (dropped for an fp32
result); the weighted path and the fallback with an fp32 result also meet the suite's 1e-5 relative tolerance."""
import importlib
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import gcn_amd
from gcn_amd import graphgen
from util import GOLDEN, bf16_assert_bound, bf16_reference, oracle_spmm, random_csr, rel_err, sym_norm_graph

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
EPS = 2.0 ** -8


def _adj(rowptr, col, val, shape, **kw):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return gcn_amd.CsrAdjacency(t(rowptr), t(col), t(val), shape, **kw)


def _bf16_features(n, k, seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return torch.randn((n, k), generator=g, device=DEV, dtype=torch.float32).to(torch.bfloat16)


def _graphs():
    rp, ci, va = sym_norm_graph(4000, 120000, seed=3)                 # ~60 entries per row: the value-free pass
    yield "sym", rp, ci, va, 4000
    rp, ci, va, n = graphgen.make_graph("reddit", device="cpu", seed=1, scale=0.02)
    yield "reddit", rp.numpy(), ci.numpy(), va.numpy(), n


_GRAPHS = {}


def _graph(name):
    if not _GRAPHS:
        for g in _graphs():
            _GRAPHS[g[0]] = g[1:]
    return _GRAPHS[name]


@pytest.mark.parametrize("name", ["sym", "reddit"])
def test_hot_path_value_free(name):
    rp, ci, va, n = _graph(name)
    adj = _adj(rp, ci, va, (n, n), symmetric=True, slices=4)
    for k in (64, 128, 192, 256, 512):
        B = _bf16_features(n, k, seed=k)
        kern = adj.main_kernel(k, dtype=torch.bfloat16)
        assert kern.startswith("gcn::spmm_group_bf16_kernel<"), (k, kern)
        Cref, absref = bf16_reference(rp, ci, va, B)
        C16 = adj.matmul_raw(B)
        assert C16.dtype == torch.bfloat16 and C16.shape == (n, k)
        bf16_assert_bound(C16, Cref, absref, bf16_out=True)
        C32 = adj.matmul_raw(B, out=torch.empty((n, k), dtype=torch.float32, device=DEV))
        bf16_assert_bound(C32, Cref, absref, bf16_out=False)
        # the bf16 result is the fp32 one rounded once
        assert torch.equal(C16, C32.to(torch.bfloat16))


def test_hot_path_value_free_on_the_automatic_slice_sets():
    """slices chosen automatically (k = 64: the slice set of 128-byte rows, built at the first call)"""
    rp, ci, va, n = _graph("reddit")
    adj = _adj(rp, ci, va, (n, n), symmetric=True)
    if adj.num_slices == 0:
        adj.enable_slicing(4)
    for k in (64, 128):
        B = _bf16_features(n, k, seed=11 + k)
        Cref, absref = bf16_reference(rp, ci, va, B)
        bf16_assert_bound(adj.matmul_raw(B), Cref, absref, bf16_out=True)
        assert adj.main_kernel(k, dtype=torch.bfloat16).startswith("gcn::spmm_group_bf16_kernel<")


def test_hot_path_weighted():
    m = n = 3000
    rp, ci, va = random_csr(m, n, m * 30, seed=5)
    adj = _adj(rp, ci, va, (m, n), slices=4)
    for k in (64, 128, 256):
        kern = adj.main_kernel(k, dtype=torch.bfloat16)
        assert kern.startswith("gcn::spmm_group_bf16_weighted_kernel<"), (k, kern)
        B = _bf16_features(n, k, seed=100 + k)
        Cref, absref = bf16_reference(rp, ci, va, B)
        C32 = adj.matmul_raw(B, out=torch.empty((m, k), dtype=torch.float32, device=DEV))
        assert rel_err(C32.cpu().numpy(), Cref) <= 1e-5
        C16 = adj.matmul_raw(B)
        bf16_assert_bound(C16, Cref, absref, bf16_out=True)


def _fallback_cases():
    rp, ci, va = random_csr(1500, 1200, 1500 * 12, seed=7, empty_rows=0.2, long_rows=((3, 60), (700, 300)))
    yield "unsliced", (rp, ci, va, (1500, 1200)), dict(slices=0)
    yield "panels", (rp, ci, va, (1500, 1200)), dict(slices=0, panels=1)
    rp2, ci2, va2 = random_csr(1000, 1000, 1000 * 20, seed=8, sorted_cols=False, long_rows=((10, 80),))
    yield "unsorted", (rp2, ci2, va2, (1000, 1000)), dict()
    rp3, ci3, va3 = sym_norm_graph(3000, 60000, seed=9)
    yield "sliced_narrow", (rp3, ci3, va3, (3000, 3000)), dict(slices=4)
    yield "empty", (np.zeros(501, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32), (500, 400)), dict(slices=0)


@pytest.mark.parametrize("case", [c[0] for c in _fallback_cases()])
def test_fallback_widths_and_plans(case):
    (rp, ci, va, shape), kw = next((c[1], c[2]) for c in _fallback_cases() if c[0] == case)
    adj = _adj(rp, ci, va, shape, **kw)
    for k in (1, 8, 16, 40, 41, 100):
        assert not adj.main_kernel(k, dtype=torch.bfloat16).startswith("gcn::spmm_group_bf16")
        B = _bf16_features(shape[1], k, seed=200 + k)
        Cref, absref = bf16_reference(rp, ci, va, B)
        C32 = adj.matmul_raw(B, out=torch.empty((shape[0], k), dtype=torch.float32, device=DEV))
        assert rel_err(C32.cpu().numpy(), Cref) <= 1e-5, (case, k)
        C16 = adj.matmul_raw(B)
        bf16_assert_bound(C16, Cref, absref, bf16_out=True)
        assert torch.equal(C16, adj.matmul_raw(B))                   # deterministic


def _keep_mask(numel, p, seed, offset):
    return gcn_amd.dropout_rows(torch.ones(numel, device=DEV), p, seed, offset) != 0


@pytest.mark.parametrize("k", [128, 40])
def test_epilogue_bias_relu_dropout(k):
    rp, ci, va = sym_norm_graph(4000, 120000, seed=3)
    n = 4000
    adj = _adj(rp, ci, va, (n, n), symmetric=True, slices=4)
    assert adj.main_kernel(k, dtype=torch.bfloat16).startswith("gcn::spmm_group_bf16") == (k == 128)
    B = _bf16_features(n, k, seed=300 + k)
    bias = torch.randn(k, device=DEV) * 0.1
    p, seed, off = 0.3, 1234, 7
    Cref, absref = bf16_reference(rp, ci, va, B)
    keep = _keep_mask(n * k, p, seed, off).reshape(n, k).cpu().numpy()
    # dropout without ReLU: the dropped positions are those of the fp32 epilogue
    C32 = adj.matmul_raw(B.float(), bias=bias, dropout=(p, seed, off))
    C16 = adj.matmul_raw(B, bias=bias, dropout=(p, seed, off))
    assert torch.equal(C16 == 0, C32 == 0)
    assert np.array_equal((C16 != 0).cpu().numpy(), keep)
    for relu in (False, True):
        for out_dtype in (torch.bfloat16, torch.float32):
            out = torch.empty((n, k), dtype=out_dtype, device=DEV)
            C = adj.matmul_raw(B, out=out, bias=bias, relu=relu, dropout=(p, seed, off))
            Z = Cref + bias.double().cpu().numpy()
            if relu:
                Z = np.maximum(Z, 0.0)
            E = np.where(keep, Z / (1.0 - p), 0.0)
            bf16_assert_bound(C, E, absref, bf16_out=out_dtype == torch.bfloat16, scale=1.0 / (1.0 - p) + 1e-3)


def test_dropout_rows_bf16_matches_the_fp32_mask():
    x = _bf16_features(777, 33, seed=4)
    y16 = gcn_amd.dropout_rows(x, 0.4, 99, 5)
    y32 = gcn_amd.dropout_rows(x.float(), 0.4, 99, 5)
    assert y16.dtype == torch.bfloat16
    assert torch.equal(y16, y32.to(torch.bfloat16))


def test_determinism_hot_path():
    rp, ci, va = sym_norm_graph(4000, 120000, seed=3)
    adj = _adj(rp, ci, va, (4000, 4000), symmetric=True, slices=4)
    B = _bf16_features(4000, 256, seed=1)
    a = adj.matmul_raw(B, bias=torch.ones(256, device=DEV), relu=True, dropout=(0.2, 5, 6))
    b = adj.matmul_raw(B, bias=torch.ones(256, device=DEV), relu=True, dropout=(0.2, 5, 6))
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))


def test_fp16_and_other_dtypes_are_refused():
    rp, ci, va = sym_norm_graph(500, 3000, seed=3)
    adj = _adj(rp, ci, va, (500, 500), symmetric=True)
    with pytest.raises(gcn_amd.GcnAmdError):
        adj.matmul_raw(torch.zeros((500, 64), dtype=torch.float16, device=DEV))
    with pytest.raises(gcn_amd.GcnAmdError):
        gcn_amd.spmm(adj, torch.zeros((500, 64), dtype=torch.float16, device=DEV))
    with pytest.raises(gcn_amd.GcnAmdError):
        gcn_amd.dropout_rows(torch.zeros(10, dtype=torch.float16, device=DEV), 0.5, 1, 1)
    with pytest.raises(ValueError):
        adj.matmul_raw(torch.zeros((500, 64), dtype=torch.bfloat16, device=DEV),
                       out=torch.empty((500, 64), dtype=torch.float16, device=DEV))


def test_install_routing_leaves_bf16_to_torch():
    spmm_mod = importlib.import_module("gcn_amd.spmm")
    a = torch.eye(8, device=DEV).to_sparse()
    assert spmm_mod._routable(a, torch.ones((8, 4), device=DEV))
    assert not spmm_mod._routable(a, torch.ones((8, 4), device=DEV, dtype=torch.bfloat16))
    assert not spmm_mod._routable(a.to(torch.bfloat16), torch.ones((8, 4), device=DEV, dtype=torch.bfloat16))


def test_autograd_non_symmetric():
    m, n, k = 2500, 1800, 128
    rp, ci, va = random_csr(m, n, m * 25, seed=12)
    adj = _adj(rp, ci, va, (m, n), symmetric=False, slices=4)
    x = _bf16_features(n, k, seed=21).requires_grad_(True)
    y = gcn_amd.spmm(adj, x)
    assert y.dtype == torch.bfloat16
    Cref, absref = bf16_reference(rp, ci, va, x.detach())
    bf16_assert_bound(y.detach(), Cref, absref, bf16_out=True)
    g = _bf16_features(m, k, seed=22)
    y.backward(g)
    assert x.grad.dtype == torch.bfloat16
    At = sp.csr_matrix((va, ci, rp), shape=(m, n)).T.tocsr()
    At.sort_indices()
    Gref, gabs = bf16_reference(At.indptr.astype(np.int32), At.indices.astype(np.int32), At.data.astype(np.float32), g)
    bf16_assert_bound(x.grad, Gref, gabs, bf16_out=True)


def _sbm_problem():
    rp, ci, _va, n = graphgen.make_sbm(4096, block=512, deg_in=24, deg_out=8, seed=3, relabel=False)
    rp, ci = rp.numpy(), ci.numpy()
    A = sp.csr_matrix((np.ones(len(ci), np.float32), ci, rp), shape=(n, n))
    A.setdiag(0); A.eliminate_zeros()
    labels = np.arange(n) // 512
    rng = np.random.default_rng(0)
    f = 64
    X = rng.standard_normal((n, f)).astype(np.float32) + 0.6 * np.eye(8)[labels] @ rng.standard_normal((8, f)).astype(np.float32)
    idx_train = rng.choice(n, 800, replace=False)
    return A, X.astype(np.float32), labels, idx_train, f


def _train(A, X, labels, idx_train, f, c, dtype, fused, iters, nhid=16, **kw):
    torch.manual_seed(15)
    model = gcn_amd.GCN(f, nhid, c, dataset="synthetic", device="cuda:0", order=None, fuse_epilogue=fused,
                        compute_dtype=dtype, **kw).to("cuda:0")
    losses = model.fit(X, A, labels, idx_train, train_iters=iters)
    return model, losses, float(model.test(idx_train, labels))


@pytest.mark.parametrize("fused", [False, True])
def test_training_bf16_planted_partition(fused):
    A, X, labels, idx_train, f = _sbm_problem()
    m16, l16, acc16 = _train(A, X, labels, idx_train, f, 8, torch.bfloat16, fused, 60)
    _m32, l32, acc32 = _train(A, X, labels, idx_train, f, 8, torch.float32, fused, 60)
    assert l16[-1] < 0.6 * l16[0]
    assert abs(acc16 - acc32) <= 0.02, (acc16, acc32)
    assert m16.gc1.weight.dtype == torch.float32 and m16.predict().dtype == torch.float32


def test_training_bf16_cora_shaped():
    g = np.load(os.path.join(GOLDEN, "gcn1_cora_shaped.npz"))
    t = np.load(os.path.join(GOLDEN, "gcn1_train_cora_shaped.npz"))
    n = int(g["n"])
    Ahat = sp.coo_matrix((g["adj_val"], (g["adj_row"], g["adj_col"])), shape=(n, n)).tocsr()
    raw = Ahat.copy(); raw.data[:] = 1.0; raw.setdiag(0); raw.eliminate_zeros()
    X = sp.coo_matrix((g["x_val"], (g["x_row"], g["x_col"])), shape=(n, int(g["nfeat"]))).tocsr()
    accs = {}
    for fused in (False, True):
        for dtype in (torch.bfloat16, torch.float32):
            _m, losses, acc = _train(raw, X, t["labels"], t["idx_train"], int(g["nfeat"]), int(g["ncls"]), dtype, fused, 200,
                                     nhid=int(g["nhid"]), dropout=0.0, lr=0.05)
            assert losses[-1] < 0.9 * losses[0], (fused, dtype, losses[0], losses[-1])
            accs[(fused, dtype)] = acc
        assert abs(accs[(fused, torch.bfloat16)] - accs[(fused, torch.float32)]) <= 0.02, accs


def test_hip_graph_with_bf16_is_refused():
    A, X, labels, idx_train, f = _sbm_problem()
    model = gcn_amd.GCN(f, 16, 8, dataset="synthetic", device="cuda:0", order=None, compute_dtype=torch.bfloat16).to("cuda:0")
    with pytest.raises(ValueError, match="not supported yet"):
        model.fit(X, A, labels, idx_train, train_iters=2, hip_graph=True)


def test_headline_graph_full_size_k128():
    rowptr, col, val, n = graphgen.make_graph("reddit", device=DEV, seed=1)
    adj = gcn_amd.CsrAdjacency(rowptr, col, val, (n, n), symmetric=True)
    k = 128
    assert adj.main_kernel(k, dtype=torch.bfloat16).startswith("gcn::spmm_group_bf16_kernel<")
    B = _bf16_features(n, k, seed=7)
    C = adj.matmul_raw(B)
    torch.cuda.synchronize()
    rows = np.sort(np.random.default_rng(0).choice(n, 2000, replace=False))
    r = torch.from_numpy(rows).to(DEV)
    rp = rowptr.long()
    start, lens = rp[r], rp[r + 1] - rp[r]
    seg = torch.repeat_interleave(torch.arange(len(rows), device=DEV), lens)
    first = torch.cumsum(lens, 0) - lens
    e = start[seg] + (torch.arange(int(lens.sum()), device=DEV) - first[seg])
    Bd = B.double()
    v, cc = val[e].double(), col[e].long()
    Cref = torch.zeros((len(rows), k), dtype=torch.float64, device=DEV).index_add_(0, seg, v[:, None] * Bd[cc])
    absref = torch.zeros_like(Cref).index_add_(0, seg, v.abs()[:, None] * Bd[cc].abs())
    bound = EPS * absref + EPS * Cref.abs() + 1e-6
    assert bool(((C[r].double() - Cref).abs() <= bound).all())

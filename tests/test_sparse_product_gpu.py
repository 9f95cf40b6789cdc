"""SparseProduct on the GPU: the product with a fixed pattern.  Its values against gcn_amd.spgemm on operands carrying the new
values, bit for bit (a random pair with repeats in A; the pair of test_spgemm_gpu whose rows reach all three accumulator
classes of the fill); the refusal of a `b` whose rows do not ascend strictly; both gradients against the fp64 dense product
within the summation bound; only the kernel calls a backward needs; a loss through spmm(P.adj, x, values=P.values(...))
against torch's dense fp64 autograd; forward + backward captured in a graph and replayed on new values; the same bits twice."""
import sys

import numpy as np
import pytest
import torch

import gcn_amd
from gcn_amd import _lib
from test_sampled_dot_cpu import _check_on_pattern, _dense_bound, _sorted
from test_spgemm_cpu import _random_csr
from test_spgemm_gpu import N as CLASS_N, class_pair
from test_spmm_gpu import TOL
from spgemm_ref import transpose_ref
from util import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
W, G = _lib.SPGEMM_WAVE_MAX, _lib.SPGEMM_BLOCK_MAX
_cache = {}


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def adj_of(x, shape, **kw):
    return gcn_amd.CsrAdjacency(t(x[0]), t(x[1]), t(x[2]), shape, **kw)


def same_bits(x, y):
    return x.shape == y.shape and torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))


def pair():
    """A [300 x 200] with repeated pairs and unsorted rows, B [200 x 400] ascending -> (a, b, adjacencies, SparseProduct)"""
    if "pair" not in _cache:
        rng = np.random.default_rng(21)
        a = _random_csr(300, 200, 0.05, rng, repeats=True)
        b = _sorted(*_random_csr(200, 400, 0.05, rng))
        A, B = adj_of(a, (300, 200), chunk_nnz=4096), adj_of(b, (200, 400))
        _cache["pair"] = (a, b, A, B, gcn_amd.SparseProduct(A, B))
    return _cache["pair"]


def check_against_spgemm(P, a, b, shape_a, shape_b, rng):
    A, B = adj_of(a, shape_a), adj_of(b, shape_b)
    c = gcn_amd.spgemm(A, B, assume_coalesced=True)
    assert (P.adj.m, P.adj.n) == (c.m, c.n) and torch.equal(P.adj.rowptr, c.rowptr) and torch.equal(P.adj.col, c.col)
    assert P.adj.mutable_values and same_bits(P.adj.val, c.val)                  # its own values are spgemm's
    assert same_bits(P.values(), c.val)                                          # None: the operands' own values
    av, bv = (t(rng.standard_normal(len(x[1])).astype(np.float32)) for x in (a, b))
    c2 = gcn_amd.spgemm(gcn_amd.CsrAdjacency(A.rowptr, A.col, av, shape_a), gcn_amd.CsrAdjacency(B.rowptr, B.col, bv, shape_b),
                        assume_coalesced=True)
    assert torch.equal(c2.col, P.adj.col)
    got = P.values(av, bv)
    assert got.dtype == torch.float32 and same_bits(got, c2.val) and not same_bits(got, c.val)
    assert same_bits(P.values(av, None), gcn_amd.spgemm(gcn_amd.CsrAdjacency(A.rowptr, A.col, av, shape_a), B, assume_coalesced=True).val)
    return c


def test_values_are_spgemms_bit_for_bit_on_a_random_pair_with_repeats_in_a():
    a, b, A, B, P = pair()
    c = check_against_spgemm(P, a, b, (300, 200), (200, 400), np.random.default_rng(22))
    assert c.nnz > 5000 and P.adj.chunk_nnz == 4096 and P.adj.symmetric is None
    assert gcn_amd.SparseProduct(A, B, symmetric=False).adj.symmetric is False


def test_values_are_spgemms_bit_for_bit_on_rows_of_all_three_accumulator_classes():
    a, b, p, ref = class_pair()
    b = _sorted(*b)                                     # (the classes depend on the lengths of B's rows, not on their order)
    products = np.minimum(ref[3], CLASS_N)
    assert (products <= W).any() and ((products > W) & (products <= G)).any() and (products > G).any()
    assert {W - 1, W, W + 1, G - 1, G, G + 1} <= set(ref[3].tolist())             # product counts around the two bounds
    m = len(a[0]) - 1
    P = gcn_amd.SparseProduct(adj_of(a, (m, p)), adj_of(b, (p, CLASS_N)))
    check_against_spgemm(P, a, b, (m, p), (p, CLASS_N), np.random.default_rng(23))


def test_a_b_whose_rows_do_not_ascend_strictly_is_refused():
    a, b, A, B, P = pair()
    rng = np.random.default_rng(24)
    unsorted = _random_csr(200, 400, 0.05, rng)
    assert np.any(np.diff(unsorted[1])[np.diff(np.repeat(np.arange(200), np.diff(unsorted[0]))) == 0] < 0)
    with pytest.raises(ValueError, match="coalesce_csr"):
        gcn_amd.SparseProduct(A, adj_of(unsorted, (200, 400)))
    rows = [b[1][b[0][i]:b[0][i + 1]] for i in range(200)]
    rows[57] = np.sort(np.concatenate([rows[57], rows[57][:1]]))                # sorted, one column twice
    rp = np.zeros(201, np.int32)
    rp[1:] = np.cumsum([len(r) for r in rows])
    repeating = (rp, np.concatenate(rows).astype(np.int32), np.ones(rp[-1], np.float32))
    with pytest.raises(ValueError, match="ascend strictly"):
        gcn_amd.SparseProduct(A, adj_of(repeating, (200, 400)))
    merged, _ = gcn_amd.coalesce_csr(adj_of(repeating, (200, 400)), "sum")      # ... and what the message says makes it pass
    assert gcn_amd.SparseProduct(A, merged).adj.nnz == P.adj.nnz


def test_both_gradients_against_the_dense_product_within_the_summation_bound():
    a, b, A, B, P = pair()
    rng = np.random.default_rng(25)
    g = (0.5 + rng.random(P.adj.nnz)).astype(np.float32)
    av, bv = t(a[2]).requires_grad_(True), t(b[2]).requires_grad_(True)
    v = P.values(av, bv)
    assert v.requires_grad
    ga, gb = torch.autograd.grad(v, (av, bv), t(g))
    c = (P.adj.rowptr.cpu().numpy(), P.adj.col.cpu().numpy(), g)
    dense, bound = _dense_bound(b, transpose_ref(*c, 400), (200, 400), (400, 300))          # B · Gᵀ
    _check_on_pattern(ga.cpu().numpy(), a, dense.T, bound.T)
    at = transpose_ref(*a, 200)
    dense, bound = _dense_bound(at, c, (200, 300), (300, 400))                              # Aᵀ · G
    _check_on_pattern(gb.cpu().numpy(), b, dense, bound)
    # the same bits at a second backward
    ga2, gb2 = torch.autograd.grad(P.values(av, bv), (av, bv), t(g))
    assert same_bits(ga, ga2) and same_bits(gb, gb2)


def test_only_the_kernel_calls_a_backward_needs(monkeypatch):
    a, b, A, B, P = pair()
    mod = sys.modules["gcn_amd.spgemm"]
    calls = []
    real = mod._sampled_dot

    def counting(pattern, *args):
        calls.append(pattern)
        return real(pattern, *args)

    monkeypatch.setattr(mod, "_sampled_dot", counting)
    g = torch.ones(P.adj.nnz, device=DEV)
    for need_a, need_b in ((True, True), (True, False), (False, True)):
        av, bv = t(a[2]).requires_grad_(need_a), t(b[2]).requires_grad_(need_b)
        del calls[:]
        v = P.values(av, bv)
        assert calls == [P.adj]
        v.backward(g)
        assert calls[1:] == [x for x, need in ((A, need_a), (B, need_b)) if need]
        assert (av.grad is not None) == need_a and (bv.grad is not None) == need_b
    del calls[:]
    v = P.values(t(a[2]), None)                         # nothing requires a gradient: no graph, one call
    assert calls == [P.adj] and not v.requires_grad
    av = t(a[2]).requires_grad_(True)
    del calls[:]
    P.values(av).sum().backward()                       # b_values None: the operand's own values, and no gradient for it
    assert calls == [P.adj, A] and av.grad is not None


def test_a_loss_through_the_spmm_against_dense_fp64_autograd():
    a, b, A, B, _ = pair()
    P = gcn_amd.SparseProduct(A, B)                     # (its own: the spmm writes the values into P.adj)
    rng = np.random.default_rng(26)
    k = 24
    X = rng.standard_normal((400, k)).astype(np.float32)
    T = rng.standard_normal((300, k)).astype(np.float32)
    av, bv, x = t(a[2]).requires_grad_(True), t(b[2]).requires_grad_(True), t(X).requires_grad_(True)
    out = gcn_amd.spmm(P.adj, x, values=P.values(av, bv))
    ((out - t(T)) ** 2).mean().backward()
    # dense: A with its repeated pairs added (index_put accumulates), B, C = A · B, out = C · X
    arows = torch.from_numpy(np.repeat(np.arange(300), np.diff(a[0]))).to(DEV)
    brows = torch.from_numpy(np.repeat(np.arange(200), np.diff(b[0]))).to(DEV)
    av64, bv64, x64 = (z.detach().double().requires_grad_(True) for z in (av, bv, x))
    Ad = torch.zeros(300, 200, dtype=torch.float64, device=DEV).index_put((arows, t(a[1]).long()), av64, accumulate=True)
    Bd = torch.zeros(200, 400, dtype=torch.float64, device=DEV).index_put((brows, t(b[1]).long()), bv64, accumulate=True)
    ref = Ad @ Bd @ x64
    ((ref - t(T).double()) ** 2).mean().backward()
    errs = [rel_err(got.detach().cpu().numpy(), want.detach().cpu().numpy())
            for got, want in ((out, ref), (av.grad, av64.grad), (bv.grad, bv64.grad), (x.grad, x64.grad))]
    print("rel. errors: out, grad a_values, grad b_values, grad x", errs)
    assert max(errs) <= TOL


def test_forward_and_backward_captured_and_replayed_on_new_values():
    a, b, A, B, P = pair()
    rng = np.random.default_rng(27)
    new = [tuple(t(rng.standard_normal(len(z[1])).astype(np.float32)) for z in (a, b)) + (t(rng.standard_normal(P.adj.nnz).astype(np.float32)),)
           for _ in range(2)]
    av, bv = t(a[2]).requires_grad_(True), t(b[2]).requires_grad_(True)
    gout = torch.ones(P.adj.nnz, device=DEV)

    def step():
        v = P.values(av, bv)
        ga, gb = torch.autograd.grad(v, (av, bv), gout)
        return v.detach(), ga, gb

    def load(values):
        with torch.no_grad():
            av.copy_(values[0])
            bv.copy_(values[1])
            gout.copy_(values[2])

    eager = []
    for values in new:
        load(values)
        eager.append(tuple(z.clone() for z in step()))
    step()                                              # (three eager calls before the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    for values, want in zip(new, eager):
        load(values)                                    # changed in place
        graph.replay()
        torch.cuda.synchronize()
        assert all(same_bits(got, w) for got, w in zip(outs, want))
    assert not same_bits(eager[0][0], eager[1][0])

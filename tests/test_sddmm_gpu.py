"""Learnable edge weights on the GPU: the SDDMM (gcn_sddmm_csr_f32, sddmm.hip) against fp64, its determinism across plans
and calls, the in-place value refresh of mutable plans (gcn_spmm_plan_update_values), autograd of spmm(values=...),
a training loop, a captured HIP graph, and the install(sparse_grad=True) routing of torch.sparse.mm.

SDDMM bound (elementwise, fp64 oracle):  |d - d*| <= 1e-5 * sum_j |A_rj * B_cj| + 1e-30."""
import importlib

import numpy as np
import pytest
import torch

import gcn_amd
from gcn_amd import graphgen
from util import check_sddmm, oracle_spmm, random_csr, sddmm_graph, sddmm_ref, sym_norm_graph, with_duplicate_entries

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
spmm_mod = importlib.import_module("gcn_amd.spmm")
KS = (1, 3, 8, 16, 32, 41, 48, 64, 100, 128, 200, 256, 512)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _adj(rp, ci, va, shape, **kw):
    return gcn_amd.CsrAdjacency(_t(rp), _t(ci), _t(va), shape, **kw)


def _plans(name):
    rp, ci, va, m, n = sddmm_graph(name)
    yield "unsliced", _adj(rp, ci, va, (m, n), slices=0)
    if name != "rect":
        yield "auto", _adj(rp, ci, va, (m, n))
    yield "sliced4", _adj(rp, ci, va, (m, n), slices=4)
    yield "panels", _adj(rp, ci, va, (m, n), slices=0, panels=1)


@pytest.mark.parametrize("name", ["rect", "sym", "reddit"])
def test_sddmm_parity_fp64(name):
    rp, ci, va, m, n = sddmm_graph(name)
    rng = np.random.default_rng(7)
    plans = dict(_plans(name))
    if name == "reddit":                                     # the sliced walk on a plan that runs the group kernels
        assert plans["sliced4"].num_slices == 4
        assert plans["sliced4"].main_kernel(128).startswith("gcn::spmm_group")
        assert plans["sliced4"].sddmm_kernel(128) == "gcn::sddmm_kernel<true, true>"
        assert plans["sliced4"].sddmm_kernel(32) == "gcn::sddmm_kernel<false, true>"
        assert plans["unsliced"].sddmm_kernel(128) == "gcn::sddmm_kernel<false, true>"
    if name == "sym":
        assert plans["auto"].has_value_factors or plans["auto"].num_slices == 0
    ks = KS if name != "reddit" else (8, 41, 128, 512)
    for k in ks:
        A = rng.standard_normal((m, k)).astype(np.float32)
        B = rng.standard_normal((n, k)).astype(np.float32)
        ref, mag = sddmm_ref(rp, ci, A, B, DEV)
        Ad, Bd = _t(A), _t(B)
        outs = {pn: adj.sddmm(Ad, Bd) for pn, adj in plans.items()}
        for pn, out in outs.items():
            check_sddmm(out, ref, mag)
        # one device function per entry: the same bits whatever plan walks it, and on a second call
        first = next(iter(outs.values()))
        for pn, out in outs.items():
            assert torch.equal(out, first), (k, pn)
        assert torch.equal(plans["unsliced"].sddmm(Ad, Bd), first)


def test_sddmm_nan_stays_in_its_row():
    rp, ci, va, m, n = sddmm_graph("reddit")
    adj = _adj(rp, ci, va, (m, n), slices=4)
    k = 128
    A = torch.randn((m, k), device=DEV)
    B = torch.randn((n, k), device=DEV)
    bad = int(np.argmax(np.diff(rp)))                       # a hub row
    A[bad, 5] = float("nan")
    out = adj.sddmm(A, B).cpu().numpy()
    rows = np.repeat(np.arange(m), np.diff(rp))
    assert np.isnan(out[rows == bad]).all()
    assert not np.isnan(out[rows != bad]).any()


def test_sddmm_k0_and_bf16():
    rp, ci, va, m, n = sddmm_graph("rect")
    adj = _adj(rp, ci, va, (m, n))
    assert torch.equal(adj.sddmm(torch.empty((m, 0), device=DEV), torch.empty((n, 0), device=DEV)),
                       torch.zeros(len(ci), device=DEV))
    A = torch.randn((m, 64), device=DEV).to(torch.bfloat16)
    B = torch.randn((n, 64), device=DEV).to(torch.bfloat16)
    out = adj.sddmm(A, B)
    assert out.dtype == torch.float32
    assert torch.equal(out, adj.sddmm(A.float(), B.float()))


def _oracle(rp, ci, w, X):
    return oracle_spmm(rp, ci, w, X).astype(np.float64)


@pytest.mark.parametrize("name", ["rect", "sym", "reddit"])
def test_refresh_matches_fresh_plan_and_oracle(name):
    """start from values that factor (a value-free plan if they stayed), refresh to new ones: every SpMM equals a fresh
    mutable plan on the new values bit for bit, and the fp64 oracle to 1e-5"""
    rp, ci, va, m, n = sddmm_graph(name)
    rng = np.random.default_rng(3)
    w2 = (rng.random(len(ci)) + 0.1).astype(np.float32)
    # ("panels_dropped": panels asked for; a mutable plan has none, so it runs unsliced — asserted below)
    kinds = {"unsliced": dict(slices=0), "sliced4": dict(slices=4), "panels_dropped": dict(slices=0, panels=1)}
    if name != "rect":
        kinds["auto"] = {}
    ones = np.ones(len(ci), np.float32) if name == "rect" else va
    for kind, kw in kinds.items():
        upd = _adj(rp, ci, ones, (m, n), mutable_values=True, **kw)
        fresh = _adj(rp, ci, w2, (m, n), mutable_values=True, **kw)
        assert upd.values_mutable and not upd.has_value_factors and upd.panel_rows == 0
        if name == "reddit" and kind == "sliced4":
            assert upd.main_kernel(128).startswith("gcn::spmm_group_weighted_kernel")
        upd.matmul_raw(torch.randn((n, 64), device=DEV))     # (a call on the old values first)
        upd.update_values(_t(w2))
        for k in (16, 40, 128):
            X = torch.randn((n, k), device=DEV)
            bias = torch.randn(k, device=DEV)
            ref = _oracle(rp, ci, w2, X.cpu().numpy())
            for fn in (lambda a: a.matmul_raw(X), lambda a: a.matmul_raw(X, bias=bias, relu=True),
                       lambda a: a.matmul_raw(X.to(torch.bfloat16), out=torch.empty((m, k), device=DEV))):
                c1, c2 = fn(upd), fn(fresh)
                assert torch.equal(c1, c2), (kind, k)
            C = upd.matmul_raw(X).cpu().numpy()
            assert np.abs(C - ref).max() <= 1e-5 * max(1.0, np.abs(ref).max()), (kind, k)
            Cb = upd.matmul_raw(X, bias=bias, relu=True).cpu().numpy()
            refb = np.maximum(ref + bias.cpu().numpy()[None, :], 0.0)
            assert np.abs(Cb - refb).max() <= 1e-5 * max(1.0, np.abs(refb).max()), (kind, k)


def test_update_values_refused_on_fixed_plan():
    rp, ci, va, m, n = sddmm_graph("reddit")
    adj = _adj(rp, ci, va, (m, n))
    X = torch.randn((n, 128), device=DEV)
    before = adj.matmul_raw(X).clone()
    with pytest.raises(gcn_amd.GcnAmdError):
        adj.update_values(torch.ones(len(ci), device=DEV))
    assert torch.equal(adj.matmul_raw(X), before)
    assert torch.equal(adj.val.cpu(), torch.from_numpy(va))


def _cpu_grads(rp, ci, w, x, shape, weight):
    rows = np.repeat(np.arange(shape[0]), np.diff(rp))
    wt = torch.tensor(w, dtype=torch.float64, requires_grad=True)
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    a = torch.sparse_coo_tensor(torch.tensor(np.stack([rows, ci])), wt, shape)
    y = torch.sparse.mm(a, xt)
    (y * torch.tensor(weight, dtype=torch.float64)).sum().backward()
    return y.detach().numpy(), wt.grad.numpy(), xt.grad.numpy()


@pytest.mark.parametrize("name", ["rect", "sym-asym", "reddit"])
def test_autograd_matches_cpu(name):
    rp, ci, va, m, n = sddmm_graph("sym" if name == "sym-asym" else name)
    rng = np.random.default_rng(11)
    w = (rng.random(len(ci)) + 0.1).astype(np.float32)     # (asymmetric learned values on a symmetric pattern)
    k = 48
    x = rng.standard_normal((n, k)).astype(np.float32)
    g = rng.standard_normal((m, k)).astype(np.float32)
    adj = _adj(rp, ci, va, (m, n), mutable_values=True, symmetric=(name == "sym-asym"))
    assert adj.transpose() is not adj
    wd = _t(w).requires_grad_(True)
    xd = _t(x).requires_grad_(True)
    y = gcn_amd.spmm(adj, xd, values=wd)
    (y * _t(g)).sum().backward()
    yr, gw, gx = _cpu_grads(rp, ci, w, x, (m, n), g)
    for got, ref in ((y.detach(), yr), (wd.grad, gw), (xd.grad, gx)):
        got = got.cpu().numpy().astype(np.float64)
        assert np.abs(got - ref).max() <= 1e-5 * max(1.0, np.abs(ref).max())


def _train(adj_or_none, rp, ci, w0, x, tgt, steps, device):
    """a few Adam steps on the edge weights; the CPU reference runs torch.sparse.mm in fp64"""
    m = len(rp) - 1
    rows = np.repeat(np.arange(m), np.diff(rp))
    if device == "cpu":
        w = torch.tensor(w0, dtype=torch.float64, requires_grad=True)
        xt, tt = torch.tensor(x, dtype=torch.float64), torch.tensor(tgt, dtype=torch.float64)
        idx = torch.tensor(np.stack([rows, ci]))
        fwd = lambda: torch.sparse.mm(torch.sparse_coo_tensor(idx, w, (m, x.shape[0])), xt)
    else:
        w = _t(w0).requires_grad_(True)
        xt, tt = _t(x), _t(tgt)
        fwd = lambda: gcn_amd.spmm(adj_or_none, xt, values=w)
    opt = torch.optim.Adam([w], lr=0.01)
    for _ in range(steps):
        opt.zero_grad()
        loss = ((fwd() - tt) ** 2).mean()
        loss.backward()
        opt.step()
    return w.detach().cpu().numpy().astype(np.float64)


def test_training_loop_follows_cpu():
    rp, ci, va, m, n = sddmm_graph("rect")
    rng = np.random.default_rng(5)
    x = rng.standard_normal((n, 32)).astype(np.float32)
    tgt = rng.standard_normal((m, 32)).astype(np.float32)
    adj = _adj(rp, ci, va, (m, n), mutable_values=True)
    w_gpu = _train(adj, rp, ci, va, x, tgt, 5, "cuda")
    w_cpu = _train(None, rp, ci, va, x, tgt, 5, "cpu")
    assert np.abs(w_gpu - w_cpu).max() <= 1e-4


def test_hip_graph_replay_equals_eager():
    rp, ci, va, m, n = sddmm_graph("reddit")
    rng = np.random.default_rng(9)
    k, steps = 64, 3
    x = _t(rng.standard_normal((n, k)).astype(np.float32))
    tgt = _t(rng.standard_normal((m, k)).astype(np.float32))

    def setup():
        adj = _adj(rp, ci, va, (m, n), mutable_values=True, slices=4)
        w = _t(va).requires_grad_(True)
        opt = torch.optim.SGD([w], lr=0.5)
        return adj, w, opt

    def step(adj, w, opt):
        opt.zero_grad(set_to_none=False)
        loss = ((gcn_amd.spmm(adj, x, values=w) - tgt) ** 2).mean()
        loss.backward()
        opt.step()

    adj, w, opt = setup()                                    # eager: one warm-up step plus `steps`
    for _ in range(1 + steps):
        step(adj, w, opt)
    w_eager = w.detach().clone()

    adj, w, opt = setup()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                               # warm-up outside the capture (builds the transpose)
        step(adj, w, opt)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step(adj, w, opt)
    for _ in range(steps):
        g.replay()
    torch.cuda.synchronize()
    assert torch.equal(w.detach(), w_eager)


def test_sparse_mm_routing_with_sparse_grad():
    rp, ci, va, m, n = sddmm_graph("rect")
    rows = np.repeat(np.arange(m), np.diff(rp))
    # (duplicates would be summed by coalesce: use the distinct pattern)
    key = rows.astype(np.int64) * n + ci
    keep = np.concatenate([[True], key[1:] != key[:-1]])
    idx = torch.tensor(np.stack([rows[keep], ci[keep]]), device=DEV)
    rng = np.random.default_rng(4)
    x0 = _t(rng.standard_normal((n, 40)).astype(np.float32))

    def run(vals, routed_as):
        a = torch.sparse_coo_tensor(idx, vals, (m, n)).coalesce().requires_grad_(True)
        x = x0.clone().requires_grad_(True)
        y = torch.sparse.mm(a, x)
        (y * y).sum().backward()
        return y.detach(), a.grad.coalesce(), x.grad

    v1 = _t(rng.random(int(keep.sum())).astype(np.float32))
    v2 = _t(rng.random(int(keep.sum())).astype(np.float32))
    want = [run(v, None) for v in (v1, v2)]                  # not installed: stock PyTorch
    try:
        gcn_amd.install()
        assert run(v1, None)[1].layout == torch.sparse_coo   # (plain install: falls through)
        assert not spmm_mod._pattern_cache
        gcn_amd.install(sparse_grad=True)
        got1 = run(v1, "hip")
        assert len(spmm_mod._pattern_cache) == 1
        adj = spmm_mod._pattern_cache[0][2]
        got2 = run(v2, "hip")
        assert len(spmm_mod._pattern_cache) == 1 and spmm_mod._pattern_cache[0][2] is adj
    finally:
        gcn_amd.uninstall()
        spmm_mod._pattern_cache.clear()
    for got, ref in zip((got1, got2), want):
        y, ga, gx = got
        yr, gar, gxr = ref
        assert ga.layout == torch.sparse_coo and torch.equal(ga.indices(), gar.indices())
        for a_, b_ in ((y, yr), (ga.values(), gar.values()), (gx, gxr)):
            assert (a_ - b_).abs().max().item() <= 1e-5 * max(1.0, b_.abs().max().item())


@pytest.mark.parametrize("slices", [0, 4])
def test_callers_values_are_never_written(slices):
    """a mutable adjacency owns its values: neither the tensor it was built from nor any values handed to it change"""
    rp, ci, va, m, n = sddmm_graph("reddit")
    rng = np.random.default_rng(21)
    w0 = _t(va)
    adj = gcn_amd.CsrAdjacency(_t(rp), _t(ci), w0, (m, n), mutable_values=True, slices=slices)
    assert adj.val.data_ptr() != w0.data_ptr()
    w1 = _t((rng.random(len(ci)) + 0.1).astype(np.float32)).requires_grad_(True)
    w2 = _t((rng.random(len(ci)) + 0.1).astype(np.float32))
    keep0, keep1 = w0.clone(), w1.detach().clone()
    x = torch.randn((n, 48), device=DEV, requires_grad=True)
    y1 = gcn_amd.spmm(adj, x, values=w1)
    y2 = gcn_amd.spmm(adj, x, values=w2)                     # a second value tensor on the same pattern
    (y1.sum() + y2.sum()).backward()
    assert torch.equal(w0, keep0) and torch.equal(w1.detach(), keep1)
    ref1 = _oracle(rp, ci, keep1.cpu().numpy(), x.detach().cpu().numpy())
    assert np.abs(y1.detach().cpu().numpy() - ref1).max() <= 1e-5 * max(1.0, np.abs(ref1).max())


def test_sparse_mm_routing_leaves_values_unchanged():
    rp, ci, va, m, n = sddmm_graph("rect")
    rows = np.repeat(np.arange(m), np.diff(rp))
    key = rows.astype(np.int64) * n + ci
    keep = np.concatenate([[True], key[1:] != key[:-1]])
    idx = torch.tensor(np.stack([rows[keep], ci[keep]]), device=DEV)
    rng = np.random.default_rng(8)
    w1 = _t(rng.random(int(keep.sum())).astype(np.float32)).requires_grad_(True)
    w2 = _t(rng.random(int(keep.sum())).astype(np.float32))
    keep1 = w1.detach().clone()
    x = torch.randn((n, 40), device=DEV)
    try:
        gcn_amd.install(sparse_grad=True)
        a1 = torch.sparse_coo_tensor(idx, w1, (m, n), is_coalesced=True)
        y1 = torch.sparse.mm(a1, x)
        a2 = torch.sparse_coo_tensor(idx, w2, (m, n), is_coalesced=True).requires_grad_(True)
        torch.sparse.mm(a2, x)                                # (no backward: nothing may write w1 anyway)
        assert len(spmm_mod._pattern_cache) == 1
        y1.sum().backward()
    finally:
        gcn_amd.uninstall()
    assert not spmm_mod._pattern_cache                        # (uninstall drops the plans)
    assert torch.equal(w1.detach(), keep1)
    ref = torch.sparse.mm(torch.sparse_coo_tensor(idx, keep1, (m, n)).double(), x.double())
    gref = torch.ones((m, 40), dtype=torch.float64, device=DEV)[torch.from_numpy(rows[keep]).to(DEV)]
    gref = (gref * x.double()[idx[1]]).sum(1)
    assert (y1.detach().double() - ref).abs().max().item() <= 1e-5 * max(1.0, ref.abs().max().item())
    assert (w1.grad.double() - gref).abs().max().item() <= 1e-5 * max(1.0, gref.abs().max().item())


def test_sparse_mm_backward_keeps_the_forwards_values_when_their_tensor_changes_in_place():
    """the COO tensor's values share the storage of the tensor it was made from, but not its version counter: the backward
    must either refuse or give the gradient of the values the forward saw (tests/test_autograd_forms_gpu.py, form 6)"""
    rp, ci, va, m, n = sddmm_graph("rect")
    rows = np.repeat(np.arange(m), np.diff(rp))
    key = rows.astype(np.int64) * n + ci
    keep = np.concatenate([[True], key[1:] != key[:-1]])
    idx = torch.tensor(np.stack([rows[keep], ci[keep]]), device=DEV)
    rng = np.random.default_rng(9)
    w0 = _t(rng.integers(1, 5, int(keep.sum())).astype(np.float32))
    x0 = _t(rng.integers(-8, 9, (n, 8)).astype(np.float32))
    g = _t(rng.integers(-8, 9, (m, 8)).astype(np.float32))

    def run(change):
        w, x = w0.clone().requires_grad_(True), x0.clone().requires_grad_(True)
        y = torch.sparse.mm(torch.sparse_coo_tensor(idx, w, (m, n), is_coalesced=True), x)
        if change:
            with torch.no_grad():
                w.neg_()
        try:
            y.backward(g)
        except RuntimeError:
            return None
        return x.grad, w.grad

    try:
        gcn_amd.install(sparse_grad=True)
        want, got = run(False), run(True)
    finally:
        gcn_amd.uninstall()
    assert got is None or (torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]))


@pytest.mark.parametrize("slices", [0, 4])
def test_plain_backward_after_update_values_uses_new_values(slices):
    """update_values(w2), then the values-free spmm: x.grad = Â(w2)ᵀ·g, against fp64 — also on
    a pattern flagged symmetric, whose learned values are not"""
    rp, ci, va, m, n = sddmm_graph("sym")
    rng = np.random.default_rng(13)
    adj = _adj(rp, ci, va, (m, n), mutable_values=True, symmetric=True, slices=slices)
    x = torch.randn((n, 64), device=DEV, requires_grad=True)
    gcn_amd.spmm(adj, x).sum().backward()                    # (builds the transpose on the old values)
    for _ in range(2):
        w2 = (rng.random(len(ci)) + 0.1).astype(np.float32)
        adj.update_values(_t(w2))
        x.grad = None
        g = torch.randn((m, 64), device=DEV)
        y = gcn_amd.spmm(adj, x)
        (y * g).sum().backward()
        rows = np.repeat(np.arange(m), np.diff(rp))
        # Âᵀ·g in fp64: the transpose's CSR from the COO of (col, row)
        order = np.lexsort((rows, ci))
        trp = np.zeros(n + 1, np.int64)
        trp[1:] = np.cumsum(np.bincount(ci, minlength=n))
        refx = _oracle(trp.astype(np.int32), rows[order].astype(np.int32), w2[order], g.cpu().numpy())
        got = x.grad.cpu().numpy()
        assert np.abs(got - refx).max() <= 1e-5 * max(1.0, np.abs(refx).max())
        refy = _oracle(rp, ci, w2, x.detach().cpu().numpy())
        assert np.abs(y.detach().cpu().numpy() - refy).max() <= 1e-5 * max(1.0, np.abs(refy).max())

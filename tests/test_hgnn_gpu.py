"""HypergraphLaplacian, HGNNConv and HGNN on the GPU: the values of G for given hyperedge weights against
gcn_amd.hypergraph_laplacian bit for bit on the identical pattern; the gradient in the weights against torch's autograd of the
dense formula in fp64, measured in units of the error the same dense formula makes when differentiated in fp32; the zero
rules; the same bits twice; the layers against the dense torch formulation; a reference checkpoint's keys; learnable
hyperedge weights on two planted clusters."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gcn_amd
from test_spgemm_cpu import dense_g, hypergraph_fixture
from test_spmm_gpu import TOL
from util import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same_bits(x, y):
    return x.shape == y.shape and torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))


def fixture_h():
    rp, ci, va, dense, w = hypergraph_fixture()
    return gcn_amd.CsrAdjacency(t(rp), t(ci), t(va), (40, 12)), dense, w


def same_pattern(a, b):
    return (a.m, a.n) == (b.m, b.n) and torch.equal(a.rowptr, b.rowptr) and torch.equal(a.col, b.col)


def dense_g_torch(H, w):
    """test_spgemm_cpu.dense_g as torch operations on one dtype, a zero degree giving a zero factor (the power is taken of a
    safe copy, so that the masked branch does not turn the gradient into NaN)"""
    one, zero = torch.ones((), dtype=H.dtype, device=H.device), torch.zeros((), dtype=H.dtype, device=H.device)
    DV, DE = (H * w).sum(1), H.sum(0)
    invDE = torch.where(DE == 0, zero, 1.0 / torch.where(DE == 0, one, DE))
    DV2 = torch.where(DV == 0, zero, torch.where(DV == 0, one, DV).pow(-0.5))
    return DV2[:, None] * ((H * (w * invDE)) @ H.T) * DV2[None, :]


def dense_of(adj, val=None):
    rows = torch.repeat_interleave(torch.arange(adj.m, device=DEV), (adj.rowptr[1:] - adj.rowptr[:-1]).long())
    out = torch.zeros(adj.m, adj.n, dtype=torch.float64, device=DEV)
    out[rows, adj.col.long()] = (adj.val if val is None else val).double()
    return out


# ---- the values ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
def test_values_are_hypergraph_laplacians_bit_for_bit_on_the_fixture(weighted):
    H, dense, w = fixture_h()
    L = gcn_amd.HypergraphLaplacian(H)
    ref = gcn_amd.hypergraph_laplacian(H, t(w) if weighted else None)
    assert same_pattern(L.adj, ref) and L.adj.mutable_values and L.adj.symmetric is True
    got = L.values(t(w) if weighted else torch.ones(12, device=DEV))
    assert got.dtype == torch.float32 and same_bits(got, ref.val)
    assert same_bits(L.adj.val, gcn_amd.hypergraph_laplacian(H).val)             # its own values: unit weights
    with pytest.raises(ValueError, match="edge_weight"):
        L.values(torch.ones(11, device=DEV))
    with pytest.raises(ValueError, match="edge_weight"):
        L.values(torch.ones(12, device=DEV, dtype=torch.float64))
    with pytest.raises(gcn_amd.GcnAmdError, match="device"):
        L.values(torch.ones(12))


def test_values_are_hypergraph_laplacians_bit_for_bit_on_a_knn_hypergraph():
    rng = np.random.default_rng(31)
    x = t(rng.standard_normal((200, 16)).astype(np.float32))
    H = gcn_amd.knn_hypergraph(x, 10)
    L = gcn_amd.HypergraphLaplacian(H)
    for w in (torch.ones(200, device=DEV), t((0.25 + rng.random(200)).astype(np.float32))):
        ref = gcn_amd.hypergraph_laplacian(H, w)
        assert same_pattern(L.adj, ref) and ref.nnz > 5000 and same_bits(L.values(w), ref.val)


# ---- the gradient ----------------------------------------------------------------------------------------------------------------
def test_gradient_in_the_weights_against_the_dense_formula():
    """|g - g64|_inf <= 4 |g32 - g64|_inf: g64 / g32 = torch autograd of the dense formula in fp64 / fp32.  Measured on the
    fixture: see the printed norms (DESIGN §4.21 quotes them)."""
    H, dense, w = fixture_h()
    L = gcn_amd.HypergraphLaplacian(H)
    rng = np.random.default_rng(32)
    cot = t(rng.standard_normal(L.adj.nnz).astype(np.float32))                   # the loss: sum of cot * G over G's entries
    wt = t(w).requires_grad_(True)
    v = L.values(wt)
    (g,) = torch.autograd.grad((v * cot).sum(), wt)
    Cd = dense_of(L.adj, cot)
    grads = {}
    for dtype in (torch.float64, torch.float32):
        wd = t(w).to(dtype).requires_grad_(True)
        Gd = dense_g_torch(t(dense).to(dtype), wd)
        if dtype == torch.float64:
            assert np.allclose(Gd.detach().cpu().numpy(), dense_g(dense, w.astype(np.float64)), rtol=1e-13, atol=0)
            assert torch.equal(Gd != 0, dense_of(L.adj, torch.ones(L.adj.nnz, device=DEV)) != 0)
        (grads[dtype],) = torch.autograd.grad((Gd * Cd.to(dtype)).sum(), wd)
    g64, g32 = grads[torch.float64], grads[torch.float32].double()
    ours, dense32 = float((g.double() - g64).abs().max()), float((g32 - g64).abs().max())
    print(f"|g - g64|_inf = {ours:.3e}   |g32 - g64|_inf = {dense32:.3e}   |g64|_inf = {float(g64.abs().max()):.3e}")
    assert g.dtype == torch.float32 and g.shape == (12,) and bool(torch.isfinite(g).all())
    assert dense32 > 0 and ours <= 4 * dense32
    # the same bits at a second backward
    (g2,) = torch.autograd.grad((L.values(wt) * cot).sum(), wt)
    assert same_bits(g, g2)


def test_a_vertex_without_hyperedge_and_a_hyperedge_of_weight_zero_give_and_get_zero():
    H, dense, w = fixture_h()
    L = gcn_amd.HypergraphLaplacian(H)
    w = w.copy()
    w[3] = 0
    wt = t(w).requires_grad_(True)
    v = L.values(wt)
    ref = gcn_amd.hypergraph_laplacian(H, t(w))
    assert same_pattern(L.adj, ref) and same_bits(v, ref.val) and bool(torch.isfinite(v).all())
    assert int(L.adj.rowptr[18] - L.adj.rowptr[17]) == 0                          # vertex 17 gives nothing
    (g,) = torch.autograd.grad(v.sum(), wt)
    assert bool(torch.isfinite(g).all()) and float(g[3]) == 0.0 and int((g != 0).sum()) == 11
    # without the hyperedge: the same gradient for the others (the hyperedge counts as absent), against the dense formula
    keep = [e for e in range(12) if e != 3]
    wd = t(w[keep]).double().requires_grad_(True)
    (gd,) = torch.autograd.grad(dense_g_torch(t(dense[:, keep]), wd).sum(), wd)
    assert rel_err(g[keep].cpu().numpy(), gd.cpu().numpy()) <= TOL


# ---- the layers ------------------------------------------------------------------------------------------------------------------
def test_layers_against_the_dense_formulation_and_a_reference_checkpoint():
    H, dense, w = fixture_h()
    G = gcn_amd.hypergraph_laplacian(H, t(w))
    Gd = dense_of(G)
    rng = np.random.default_rng(33)
    x = t(rng.standard_normal((40, 20)).astype(np.float32))
    torch.manual_seed(0)
    conv = gcn_amd.HGNNConv(20, 8).to(DEV)
    assert conv.weight.shape == (20, 8) and conv.bias.shape == (8,)
    assert float(conv.weight.detach().abs().max()) <= 1 / np.sqrt(8) and float(conv.bias.detach().abs().max()) <= 1 / np.sqrt(8)
    ref = Gd @ (x.double() @ conv.weight.detach().double() + conv.bias.detach().double())       # the bias BEFORE the aggregation
    assert rel_err(conv(x, G).detach().cpu().numpy(), ref.cpu().numpy()) <= TOL
    nobias = gcn_amd.HGNNConv(20, 8, with_bias=False).to(DEV)
    assert nobias.bias is None and [n for n, _ in nobias.named_parameters()] == ["weight"]
    model = gcn_amd.HGNN(20, 5, 16).to(DEV).eval()
    assert sorted(n for n, _ in model.named_parameters()) == ["hgc1.bias", "hgc1.weight", "hgc2.bias", "hgc2.weight"]
    state = {"hgc1.weight": torch.randn(20, 16), "hgc1.bias": torch.randn(16), "hgc2.weight": torch.randn(16, 5),
             "hgc2.bias": torch.randn(5)}                                          # the reference's key names
    model.load_state_dict(state, strict=True)
    p = {k: v.to(DEV).double() for k, v in state.items()}
    hid = torch.relu(Gd @ (x.double() @ p["hgc1.weight"] + p["hgc1.bias"]))
    ref = Gd @ (hid @ p["hgc2.weight"] + p["hgc2.bias"])
    out = model(x, G)
    assert isinstance(out, torch.Tensor) and out.shape == (40, 5)                  # the logits only
    assert rel_err(out.detach().cpu().numpy(), ref.cpu().numpy()) <= TOL
    assert same_bits(out, model(x, G))                                             # evaluation: no dropout
    model.train()
    assert not same_bits(out, model(x, G))                                         # training: dropout follows self.training


def clusters():
    """two planted clusters of 100 points each in 8 dimensions, their kNN hypergraph (k = 10) and labels"""
    rng = np.random.default_rng(34)
    x = rng.standard_normal((200, 8)).astype(np.float32)
    x[:100] += 1.0
    x[100:] -= 1.0
    order = rng.permutation(200)
    labels = (np.arange(200) >= 100).astype(np.int64)[order]
    x = t(x[order])
    return x, gcn_amd.knn_hypergraph(x, 10), t(labels)


def test_learnable_hyperedge_weights_train():
    x, H, labels = clusters()
    L = gcn_amd.HypergraphLaplacian(H)
    torch.manual_seed(1)
    model = gcn_amd.HGNN(8, 2, 16, dropout=0.0, learn_edge_weights=True, n_edges=200).to(DEV)
    assert model.log_edge_weight.shape == (200,) and float(model.log_edge_weight.detach().abs().max()) == 0
    opt = torch.optim.Adam(model.parameters(), lr=0.02)
    losses = []
    for _ in range(31):                                                            # the loss of step 0 and of 30 steps after it
        opt.zero_grad()
        loss = F.cross_entropy(model(x, L), labels)
        loss.backward()
        losses.append(float(loss))
        opt.step()
    print("training loss at step 0 and after 30 steps", losses[0], losses[-1])
    assert losses[-1] < losses[0]
    lw = model.log_edge_weight.detach()
    assert bool(torch.isfinite(lw).all()) and float(lw.abs().max()) > 0 and int((lw != 0).sum()) > 100
    with pytest.raises(TypeError):
        model(x, L.adj)
    with pytest.raises(ValueError, match="n_edges"):
        gcn_amd.HGNN(8, 2, 16, learn_edge_weights=True)


def test_fixed_weights_follow_a_dense_torch_hgnn():
    x, H, labels = clusters()
    G = gcn_amd.hypergraph_laplacian(H)
    Gd = dense_of(G)
    torch.manual_seed(2)
    model = gcn_amd.HGNN(8, 2, 16, dropout=0.0).to(DEV)
    assert not hasattr(model, "log_edge_weight") and len(list(model.parameters())) == 4
    names = ["hgc1.weight", "hgc1.bias", "hgc2.weight", "hgc2.bias"]
    ours = dict(model.named_parameters())
    dense = {k: ours[k].detach().double().clone().requires_grad_(True) for k in names}
    opt, opt_d = torch.optim.SGD(model.parameters(), lr=0.2), torch.optim.SGD(list(dense.values()), lr=0.2)
    for step in range(5):
        opt.zero_grad()
        loss = F.cross_entropy(model(x, G), labels)
        loss.backward()
        opt.step()
        opt_d.zero_grad()
        hid = torch.relu(Gd @ (x.double() @ dense["hgc1.weight"] + dense["hgc1.bias"]))
        loss_d = F.cross_entropy(Gd @ (hid @ dense["hgc2.weight"] + dense["hgc2.bias"]), labels)
        loss_d.backward()
        opt_d.step()
        assert abs(float(loss) - float(loss_d)) <= TOL * abs(float(loss_d)), step
    for k in names:
        assert rel_err(ours[k].detach().cpu().numpy(), dense[k].detach().cpu().numpy()) <= TOL, k

"""The GATv2 score without a GPU: the three symbols are declared, exported and bound, the C ABI rejects bad sizes before it
reads a pointer and launches nothing for an empty problem, its workspace query is the documented formula and leaves
gcn_heads_ws_bytes alone, gatv2_scores refuses CPU tensors and wrong shapes, GraphAttentionV2 constructs with the parameters
it documents — and the host twin of tests/gatv2_ref.py agrees with torch fp64 autograd of the dense formulation."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import gatv2_ref
import gcn_amd
import heads_ref
from gcn_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID = 0, 1
NULL = ctypes.c_void_p()
JUNK = ctypes.c_void_p(64)                        # a non-null pointer that must never be read
NAMES = ["gcn_gatv2_ws_bytes", "gcn_gatv2_scores_csr_f32", "gcn_gatv2_scores_backward_csr_f32"]


def calls(lib, rowptr, m, nnz, heads, k, p=JUNK, ws=JUNK, ws_bytes=1 << 40, perm=NULL, act=NULL):
    """the forward and the backward on the same sizes, all data pointers p -> list of (name, status)"""
    return [
        ("scores", lib.gcn_gatv2_scores_csr_f32(rowptr, p, m, nnz, heads, k, p, p, p, 0.2, p, ws, ws_bytes, NULL)),
        ("backward", lib.gcn_gatv2_scores_backward_csr_f32(rowptr, p, perm, m, nnz, heads, k, p, p, p, 0.2, p, p, act, ws, ws_bytes,
                                                           NULL)),
    ]


def test_symbols_are_declared_exported_and_bound():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "gcn_spmm.h")).read()
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert callable(gcn_amd.gatv2_scores) and issubclass(gcn_amd.GraphAttentionV2, torch.nn.Module)


def test_bad_sizes_are_rejected_before_any_pointer_is_read():
    lib = _lib.load()
    for heads in (0, -3):
        assert all(st == INVALID for _n, st in calls(lib, JUNK, 4, 8, heads, 8)), heads
    assert all(st == INVALID for _n, st in calls(lib, JUNK, 4, 1 << 28, 8, 64))                 # nnz * H >= 2^31
    assert all(st == INVALID for _n, st in calls(lib, JUNK, 4, (1 << 31) - 1, 1 << 10, 1 << 10))
    assert all(st == INVALID for _n, st in calls(lib, JUNK, -1, 8, 2, 8))                       # negative sizes
    assert all(st == INVALID for _n, st in calls(lib, JUNK, 4, -1, 2, 8))
    for k in (0, -8, 1, 3, 7, 9, 16 * 65535 + 2):                                               # k: a positive multiple of heads, <= 16 * 65535
        assert all(st == INVALID for _n, st in calls(lib, JUNK, 4, 8, 2, k)), k
    need = ctypes.c_size_t(0)
    assert lib.gcn_gatv2_ws_bytes(4, 8, 2, 7, ctypes.byref(need)) == INVALID
    assert lib.gcn_gatv2_ws_bytes(4, 8, 0, 8, ctypes.byref(need)) == INVALID
    assert lib.gcn_gatv2_ws_bytes(-1, 8, 2, 8, ctypes.byref(need)) == INVALID
    assert lib.gcn_gatv2_ws_bytes(4, 1 << 28, 8, 64, ctypes.byref(need)) == INVALID
    assert lib.gcn_gatv2_ws_bytes(4, 8, 2, 8, None) == INVALID


def test_null_pointers_and_a_short_workspace_are_rejected():
    lib = _lib.load()
    assert all(st == INVALID for _n, st in calls(lib, NULL, 4, 8, 2, 8))                        # no row pointer
    assert all(st == INVALID for _n, st in calls(lib, JUNK, 4, 8, 2, 8, p=NULL))                # no operands
    assert all(st == INVALID for _n, st in calls(lib, JUNK, 4, 8, 2, 8, p=NULL, perm=JUNK, act=JUNK))
    assert all(st == INVALID for _n, st in calls(lib, JUNK, 4, 8, 2, 8, ws=NULL))               # no workspace
    assert all(st == INVALID for _n, st in calls(lib, JUNK, 4, 8, 2, 8, ws_bytes=8))            # a short one


def test_workspace_size_is_the_documented_formula_and_the_family_query_is_unchanged():
    lib = _lib.load()
    need, fam = ctypes.c_size_t(0), ctypes.c_size_t(0)
    for m, nnz, heads, k in [(10, 100, 1, 16), (10, 100000, 8, 64), (5, 1 << 20, 16, 256), (3, 9000, 3, 15), (7, 4096, 2, 8),
                             (7, 4097, 2, 8)]:
        assert lib.gcn_gatv2_ws_bytes(m, nnz, heads, k, ctypes.byref(need)) == OK
        assert need.value == 16 + 2 * 8 * k * ((nnz + 4095) // 4096)
        # one byte less is refused (the pointers are never reached), the exact size passes the size checks: with no
        # operands the call then stops at the null pointers
        assert all(st == INVALID for _n, st in calls(lib, JUNK, m, nnz, heads, k, ws_bytes=need.value - 1))
        assert lib.gcn_heads_ws_bytes(m, nnz, heads, k, ctypes.byref(fam)) == OK
        assert fam.value == max(16 + 16 * heads * ((nnz + 8191) // 8192), 16 + 8 * k * ((nnz + 4095) // 4096))


def test_empty_problems_return_ok_and_launch_nothing():
    """no device in this process: a launch or a memset node would come back as a HIP error, and a pointer read would fault"""
    lib = _lib.load()
    for m, nnz in [(0, 0), (0, 8), (4, 0)]:
        got = calls(lib, JUNK, m, nnz, 2, 8, ws=NULL, ws_bytes=0)
        assert all(st == OK for _n, st in got), (m, nnz, got)


def _fake_adj(m=4, n=5, nnz=6):
    adj = gcn_amd.CsrAdjacency.__new__(gcn_amd.CsrAdjacency)      # (no device: the operand checks come first)
    adj.m, adj.n, adj.nnz, adj.mutable_values = m, n, nnz, False
    return adj


def test_cpu_tensors_wrong_ranks_and_wrong_shapes_raise():
    adj = _fake_adj()
    z = torch.zeros
    with pytest.raises(gcn_amd.GcnAmdError):
        gcn_amd.gatv2_scores(adj, z(4, 8), z(5, 8), z(2, 4))
    with pytest.raises(gcn_amd.GcnAmdError):
        gcn_amd.gatv2_scores(adj, z(4, 8, dtype=torch.float64), z(5, 8, dtype=torch.float64), z(2, 4, dtype=torch.float64))
    bad = [
        lambda: gcn_amd.gatv2_scores(adj, z(5, 8), z(5, 8), z(2, 4)),        # h_dst has m rows
        lambda: gcn_amd.gatv2_scores(adj, z(4, 8), z(4, 8), z(2, 4)),        # h_src has n rows
        lambda: gcn_amd.gatv2_scores(adj, z(4, 8), z(5, 6), z(2, 4)),        # widths differ
        lambda: gcn_amd.gatv2_scores(adj, z(4, 8), z(5, 8), z(2, 3)),        # H * F is not the width
        lambda: gcn_amd.gatv2_scores(adj, z(4, 8), z(5, 8), z(8)),           # att must be [H, F]
        lambda: gcn_amd.gatv2_scores(adj, z(4, 8), z(5, 8), z(0, 4)),
        lambda: gcn_amd.gatv2_scores(adj, z(4, 8), z(5, 8), z(2, 0)),
        lambda: gcn_amd.gatv2_scores(adj, z(4, 8, 1), z(5, 8), z(2, 4)),     # rank 3
        lambda: gcn_amd.gatv2_scores(adj, z(4, 8), None, z(2, 4)),
    ]
    for f in bad:
        with pytest.raises(ValueError):
            f()
    with pytest.raises(TypeError):
        gcn_amd.gatv2_scores(object(), z(4, 8), z(5, 8), z(2, 4))


def test_graph_attention_v2_constructs_with_the_documented_parameters():
    torch.manual_seed(0)
    layer = gcn_amd.GraphAttentionV2(12, 8, heads=4)
    assert sorted(layer.state_dict()) == ["att", "bias", "weight_dst", "weight_src"]
    assert layer.weight_src.shape == layer.weight_dst.shape == (12, 32) and layer.att.shape == (4, 8)
    assert layer.bias.shape == (32,) and int(torch.count_nonzero(layer.bias)) == 0
    assert not torch.equal(layer.weight_src, layer.weight_dst)
    bound = (6.0 / (12 + 32)) ** 0.5                                 # Glorot uniform
    assert 0.5 * bound < float(layer.weight_src.detach().abs().max()) <= bound
    assert float(layer.att.detach().abs().max()) <= (6.0 / (4 + 8)) ** 0.5
    shared = gcn_amd.GraphAttentionV2(12, 8, heads=4, concat=False, share_weights=True)
    assert sorted(shared.state_dict()) == ["att", "bias", "weight_src"] and shared.weight_dst is None
    assert shared.bias.shape == (8,) and "shared" in repr(shared) and "shared" not in repr(layer)
    nb = gcn_amd.GraphAttentionV2(12, 8, heads=2, with_bias=False)
    assert nb.bias is None and sorted(nb.state_dict()) == ["att", "weight_dst", "weight_src"]
    layer.load_state_dict(gcn_amd.GraphAttentionV2(12, 8, heads=4).state_dict())
    with pytest.raises(ValueError):
        gcn_amd.GraphAttentionV2(12, 8, heads=0)
    with pytest.raises(ValueError):                                  # the operand rows are checked before any kernel
        layer((torch.zeros(5, 12), torch.zeros(5, 12)), _fake_adj())


# ---- the host twin against torch fp64 autograd of the dense formulation -------------------------------------------------------
def test_the_twin_agrees_with_dense_torch_fp64_autograd():
    rng = np.random.default_rng(0)
    lens = np.array([3, 0, 1, 7, 0, 0, 12, 2])
    rowptr = np.concatenate([[0], np.cumsum(lens)])
    n = 9
    col = rng.integers(0, n, rowptr[-1])
    m, nnz, H, F = len(rowptr) - 1, len(col), 3, 5
    row = heads_ref.entry_rows(rowptr)
    hd, hs = rng.standard_normal((m, H * F)), rng.standard_normal((n, H * F))
    att, g = rng.standard_normal((H, F)), rng.standard_normal((nnz, H))
    for slope in (0.2, 1.5):
        a, b, w = (torch.from_numpy(t).requires_grad_(True) for t in (hd, hs, att))
        s = (torch.nn.functional.leaky_relu(a[row] + b[col], slope).view(nnz, H, F) * w).sum(-1)
        s.backward(torch.from_numpy(g))
        assert np.allclose(gatv2_ref.scores(rowptr, col, hd, hs, att, slope), s.detach().numpy(), rtol=1e-12, atol=1e-14)
        gd, gs, act, ga = gatv2_ref.backward(rowptr, col, n, hd, hs, att, slope, g)
        assert np.allclose(gd, a.grad.numpy(), rtol=1e-10, atol=1e-14)
        assert np.allclose(gs, b.grad.numpy(), rtol=1e-10, atol=1e-14)
        assert np.allclose(ga, w.grad.numpy(), rtol=1e-10, atol=1e-14)
        assert np.allclose(act.sum(0).reshape(H, F), ga, rtol=1e-12, atol=1e-14)
        assert gd.shape == (m, H * F) and gs.shape == (n, H * F) and not gd[[1, 4, 5]].any()       # empty rows: zeros
        # the magnitudes bound the values they belong to
        assert (np.abs(gatv2_ref.scores(rowptr, col, hd, hs, att, slope)) <=
                gatv2_ref.scores_magnitude(rowptr, col, hd, hs, att, slope) + 1e-12).all()
        md, ms, ma = gatv2_ref.backward_magnitudes(rowptr, col, n, hd, hs, att, slope, g)
        assert (np.abs(gd) <= md + 1e-12).all() and (np.abs(gs) <= ms + 1e-12).all() and (np.abs(act) <= ma + 1e-12).all()
    # t == 0: the value is 0 and the derivative is the slope
    hd0, hs0 = np.zeros((m, H * F)), np.zeros((n, H * F))
    assert not gatv2_ref.scores(rowptr, col, hd0, hs0, att, 0.2).any()
    gd0 = gatv2_ref.backward(rowptr, col, n, hd0, hs0, att, 0.25, np.ones((nnz, H)))[0]
    assert np.allclose(gd0, 0.25 * att.reshape(1, -1) * lens[:, None])

"""The head-batched attention primitives without a GPU: the symbols are exported and bound, the C ABI rejects bad sizes before
it reads a pointer and launches nothing for an empty problem, the Python functions refuse CPU tensors and wrong shapes, and
GraphAttention(head_batched=True) is the same module as the loop form as far as its parameters go.  Plus the host twins of
tests/heads_ref.py against independent formulations (torch in fp64)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import gcn_amd
import heads_ref
from gcn_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID = 0, 1
NULL = ctypes.c_void_p()
JUNK = ctypes.c_void_p(64)                        # a non-null pointer that must never be read
NAMES = ["gcn_heads_ws_bytes", "gcn_edge_softmax_heads_csr_f32", "gcn_edge_softmax_heads_backward_csr_f32",
         "gcn_gat_edge_softmax_heads_csr_f32", "gcn_gat_edge_softmax_heads_backward_csr_f32", "gcn_segment_sum_heads_csr_f32",
         "gcn_spmm_heads_csr_f32", "gcn_sddmm_heads_csr_f32"]


def calls(lib, rowptr, m, nnz, heads, k, p=JUNK, ws=JUNK, ws_bytes=1 << 40):
    """every entry point on the same sizes, all data pointers p -> list of (name, status)"""
    return [
        ("softmax", lib.gcn_edge_softmax_heads_csr_f32(rowptr, m, nnz, heads, p, p, ws, ws_bytes, NULL)),
        ("softmax_bwd", lib.gcn_edge_softmax_heads_backward_csr_f32(rowptr, m, nnz, heads, p, p, p, ws, ws_bytes, NULL)),
        ("gat", lib.gcn_gat_edge_softmax_heads_csr_f32(rowptr, p, m, nnz, heads, p, p, 0.2, p, ws, ws_bytes, NULL)),
        ("gat_bwd", lib.gcn_gat_edge_softmax_heads_backward_csr_f32(rowptr, p, m, nnz, heads, p, p, 0.2, p, p, p, p, ws, ws_bytes,
                                                                    NULL)),
        ("segsum", lib.gcn_segment_sum_heads_csr_f32(rowptr, m, nnz, heads, p, NULL, p, ws, ws_bytes, NULL)),
        ("spmm", lib.gcn_spmm_heads_csr_f32(rowptr, p, NULL, m, nnz, heads, k, p, p, p, ws, ws_bytes, NULL)),
        ("sddmm", lib.gcn_sddmm_heads_csr_f32(rowptr, p, m, nnz, heads, k, p, p, p, ws, ws_bytes, NULL)),
    ]


def test_symbols_are_declared_exported_and_bound():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "gcn_spmm.h")).read()
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    from gcn_amd import build as gbuild
    assert "multihead.hip" in gbuild.SOURCES
    for fn in ("spmm_heads", "sddmm_heads", "edge_softmax", "gat_edge_softmax", "segment_sum"):
        assert callable(getattr(gcn_amd, fn))


def test_bad_sizes_are_rejected_before_any_pointer_is_read():
    lib = _lib.load()
    for heads in (0, -3):
        assert all(st == INVALID for _n, st in calls(lib, JUNK, 4, 8, heads, 8)), heads
    # nnz * H >= 2^31 (H = 8: from nnz = 2^28 on), with pointers that would fault if read
    assert all(st == INVALID for _n, st in calls(lib, JUNK, 4, 1 << 28, 8, 64))
    assert all(st == INVALID for _n, st in calls(lib, JUNK, 4, (1 << 31) - 1, 1 << 10, 1 << 10))
    # negative sizes
    assert all(st == INVALID for _n, st in calls(lib, JUNK, -1, 8, 2, 8))
    assert all(st == INVALID for _n, st in calls(lib, JUNK, 4, -1, 2, 8))
    # k must be a positive multiple of heads (the two calls that take k)
    for k in (0, -8, 3, 7, 9):
        got = dict(calls(lib, JUNK, 4, 8, 2, k))
        assert got["spmm"] == INVALID and got["sddmm"] == INVALID, k
    need = ctypes.c_size_t(0)
    assert lib.gcn_heads_ws_bytes(4, 8, 2, 7, ctypes.byref(need)) == INVALID
    assert lib.gcn_heads_ws_bytes(4, 8, 0, 8, ctypes.byref(need)) == INVALID
    assert lib.gcn_heads_ws_bytes(4, 1 << 28, 8, 64, ctypes.byref(need)) == INVALID
    assert lib.gcn_heads_ws_bytes(4, 8, 2, 8, None) == INVALID


def test_null_pointers_and_a_short_workspace_are_rejected():
    lib = _lib.load()
    assert all(st == INVALID for _n, st in calls(lib, NULL, 4, 8, 2, 8))                       # no row pointer
    assert all(st == INVALID for _n, st in calls(lib, JUNK, 4, 8, 2, 8, p=NULL))               # no operands
    assert all(st == INVALID for _n, st in calls(lib, JUNK, 4, 8, 2, 8, ws=NULL))              # no workspace
    assert all(st == INVALID for _n, st in calls(lib, JUNK, 4, 8, 2, 8, ws_bytes=8))           # a short one


def test_workspace_size_covers_every_entry_point():
    lib = _lib.load()
    need = ctypes.c_size_t(0)
    for m, nnz, heads, k in [(10, 100, 1, 16), (10, 100000, 8, 64), (5, 1 << 20, 16, 256), (3, 9000, 3, 15)]:
        assert lib.gcn_heads_ws_bytes(m, nnz, heads, k, ctypes.byref(need)) == OK
        edge = 16 + 16 * heads * ((nnz + 8191) // 8192)
        spmm = 16 + 8 * k * ((nnz + 4095) // 4096)
        assert need.value == max(edge, spmm)
        # one byte less than an entry point's own need is refused (the pointers are never reached)
        got = dict(calls(lib, JUNK, m, nnz, heads, k, p=NULL, ws_bytes=edge - 1))
        assert got["softmax"] == got["gat_bwd"] == got["segsum"] == INVALID
        assert dict(calls(lib, JUNK, m, nnz, heads, k, p=NULL, ws_bytes=spmm - 1))["spmm"] == INVALID


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


def test_cpu_tensors_wrong_ranks_and_wrong_lengths_raise():
    adj = _fake_adj()
    z = torch.zeros
    with pytest.raises(gcn_amd.GcnAmdError):
        gcn_amd.edge_softmax(adj, z(6, 2))
    with pytest.raises(gcn_amd.GcnAmdError):
        gcn_amd.gat_edge_softmax(adj, z(4, 2), z(5, 2))
    with pytest.raises(gcn_amd.GcnAmdError):
        gcn_amd.spmm_heads(adj, z(5, 8), z(6, 2))
    with pytest.raises(gcn_amd.GcnAmdError):
        gcn_amd.sddmm_heads(adj, z(4, 8), z(5, 8), 2)
    with pytest.raises(gcn_amd.GcnAmdError):
        gcn_amd.segment_sum(z(5, dtype=torch.int32), z(6, 2))
    with pytest.raises(gcn_amd.GcnAmdError):
        gcn_amd.edge_softmax(adj, z(6, 2, dtype=torch.float64))
    bad = [
        lambda: gcn_amd.edge_softmax(adj, z(7, 2)),                   # not nnz entries
        lambda: gcn_amd.edge_softmax(adj, z(6, 2, 1)),                # rank 3
        lambda: gcn_amd.edge_softmax(adj, z(6, 0)),                   # no head
        lambda: gcn_amd.gat_edge_softmax(adj, z(4, 2), z(5, 3)),      # head counts differ
        lambda: gcn_amd.gat_edge_softmax(adj, z(4, 2), z(5)),         # ranks differ
        lambda: gcn_amd.gat_edge_softmax(adj, z(5, 2), z(5, 2)),      # a_dst has m rows
        lambda: gcn_amd.spmm_heads(adj, z(5, 8), z(6)),               # values must be [nnz, H]
        lambda: gcn_amd.spmm_heads(adj, z(5, 7), z(6, 2)),            # k not a multiple of H
        lambda: gcn_amd.spmm_heads(adj, z(4, 8), z(6, 2)),            # x has n rows
        lambda: gcn_amd.spmm_heads(adj, z(5, 8), z(5, 2)),            # values has nnz rows
        lambda: gcn_amd.sddmm_heads(adj, z(4, 8), z(5, 8), 3),        # k not a multiple of heads
        lambda: gcn_amd.sddmm_heads(adj, z(4, 8), z(5, 8), 0),
        lambda: gcn_amd.sddmm_heads(adj, z(4, 8), z(5, 4), 2),        # widths differ
        lambda: gcn_amd.sddmm_heads(adj, z(5, 8), z(5, 8), 2),        # a has m rows
        lambda: gcn_amd.sddmm_heads(adj, z(4, 8), z(5, 8, 1), 2),
        lambda: gcn_amd.segment_sum(z(5, dtype=torch.int32), z(6, 2, 2)),
        lambda: gcn_amd.segment_sum(z(5, dtype=torch.int32), z(6, 2), perm=z(6, 2, dtype=torch.int32)),
    ]
    for i, f in enumerate(bad):
        with pytest.raises(ValueError):
            f()
        assert i >= 0
    with pytest.raises(TypeError):
        gcn_amd.spmm_heads(object(), z(5, 8), z(6, 2))
    with pytest.raises(TypeError):
        gcn_amd.sddmm_heads(object(), z(4, 8), z(5, 8), 2)


def test_the_1d_forms_keep_their_checks():
    adj = _fake_adj()
    with pytest.raises(ValueError):
        gcn_amd.edge_softmax(adj, torch.zeros(7))
    with pytest.raises(gcn_amd.GcnAmdError):
        gcn_amd.edge_softmax(adj, torch.zeros(6))
    with pytest.raises(gcn_amd.GcnAmdError):                          # (1-D GAT still asks for a mutable adjacency)
        gcn_amd.gat_edge_softmax(adj, torch.zeros(4), torch.zeros(5))


def test_head_batched_layer_constructs_and_shares_the_state_dict():
    torch.manual_seed(0)
    loop = gcn_amd.GraphAttention(12, 8, heads=4, concat=False)
    batched = gcn_amd.GraphAttention(12, 8, heads=4, concat=False, head_batched=True)
    assert loop.head_batched is False and batched.head_batched is True
    assert gcn_amd.GraphAttention(12, 8).head_batched is False                       # the default stays the loop
    assert "head-batched" in repr(batched) and "head-batched" not in repr(loop)
    sd = loop.state_dict()
    assert sorted(sd) == sorted(batched.state_dict()) == ["att_dst", "att_src", "bias", "weight"]
    batched.load_state_dict(sd)
    for k, v in batched.state_dict().items():
        assert torch.equal(v, sd[k]) and v.shape == sd[k].shape
    loop.load_state_dict(batched.state_dict())                                       # and back
    nb = gcn_amd.GraphAttention(12, 8, heads=2, with_bias=False, head_batched=True)
    assert nb.bias is None and sorted(nb.state_dict()) == ["att_dst", "att_src", "weight"]


# ---- the host twins against independent formulations ---------------------------------------------------------------------
def _small():
    rng = np.random.default_rng(0)
    lens = np.array([3, 0, 1, 7, 0, 0, 12, 2])
    rowptr = np.concatenate([[0], np.cumsum(lens)])
    n = 9
    col = rng.integers(0, n, rowptr[-1])
    return rowptr, col, n, rng


def test_the_twins_agree_with_dense_torch_fp64():
    rowptr, col, n, rng = _small()
    m, nnz, H, F = len(rowptr) - 1, len(col), 3, 5
    row = heads_ref.entry_rows(rowptr)
    s = rng.standard_normal((nnz, H))
    x, a = rng.standard_normal((n, H * F)), rng.standard_normal((m, H * F))
    v = rng.standard_normal((nnz, H))
    # softmax and its backward through autograd
    st = torch.from_numpy(s).requires_grad_(True)
    pt = torch.zeros(nnz, H, dtype=torch.float64)
    for r in range(m):
        if rowptr[r + 1] > rowptr[r]:
            pt[rowptr[r]:rowptr[r + 1]] = torch.softmax(st[rowptr[r]:rowptr[r + 1]], dim=0)
    g = rng.standard_normal((nnz, H))
    pt.backward(torch.from_numpy(g))
    p = heads_ref.edge_softmax(rowptr, s)
    assert np.allclose(p, pt.detach().numpy(), rtol=1e-12, atol=0)
    assert np.allclose(heads_ref.edge_softmax_backward(rowptr, p, g), st.grad.numpy(), rtol=1e-10, atol=1e-14)
    # all -inf (row, head) -> zeros; it leaves the other heads alone
    s2 = s.copy()
    s2[rowptr[3]:rowptr[4], 1] = -np.inf
    p2 = heads_ref.edge_softmax(rowptr, s2)
    assert (p2[rowptr[3]:rowptr[4], 1] == 0).all() and np.array_equal(p2[:, [0, 2]], p[:, [0, 2]])
    # SpMM, its transposed form and the SDDMM against dense per-head matrices
    out = heads_ref.spmm_heads(rowptr, col, None, v, x, H)
    sd = heads_ref.sddmm_heads(rowptr, col, a, x, H)
    trp, trow, tperm = heads_ref.transpose_pattern(rowptr, col, n)
    gx = heads_ref.spmm_heads(trp, trow, tperm, v, a, H)
    for h in range(H):
        D = np.zeros((m, n))
        np.add.at(D, (row, col), v[:, h])
        sl = slice(h * F, (h + 1) * F)
        assert np.allclose(out[:, sl], D @ x[:, sl], rtol=1e-12, atol=1e-14)
        assert np.allclose(gx[:, sl], D.T @ a[:, sl], rtol=1e-12, atol=1e-14)
        assert np.allclose(sd[:, h], (a[:, sl] @ x[:, sl].T)[row, col], rtol=1e-12, atol=1e-14)
    assert np.array_equal(col[tperm], np.sort(col)) and np.array_equal(row[tperm], trow)
    assert np.allclose(heads_ref.segment_sum(trp, v, tperm), np.stack([np.bincount(col, v[:, h], n) for h in range(H)], 1))
    # the fused scores
    ad, asr = rng.standard_normal((m, H)).astype(np.float32), rng.standard_normal((n, H)).astype(np.float32)
    sc = heads_ref.gat_scores(rowptr, col, ad, asr, 0.2)
    want = torch.nn.functional.leaky_relu(torch.from_numpy(ad)[row] + torch.from_numpy(asr)[col], 0.2).numpy()
    assert np.array_equal(sc, want)
    ds, gd = heads_ref.gat_edge_softmax_backward(rowptr, col, ad, asr, 0.2, p, g)
    assert np.allclose(gd, heads_ref.row_sums(rowptr, ds))

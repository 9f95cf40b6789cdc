"""The sparse x sparse product without a GPU: the three entry points are exported and bound, the limits of the binding are
the header's, the calls refuse bad arguments before anything is launched, the Python layer checks its arguments in the
documented order, and the numpy twins the GPU tests compare with (tests/spgemm_ref.py) agree with scipy's product within
the summation bound and with the dense fp64 formula of the hypergraph Laplacian."""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import gcn_amd
from gcn_amd import _lib
from spgemm_ref import hypergraph_laplacian_ref, sorted_merged_ref, spgemm_ref, transpose_ref
from util import ROOT

INVALID = 1                                            # GCN_ERR_INVALID_ARG
SYMBOLS = [("gcn_spgemm_ws_bytes", 3), ("gcn_spgemm_count_csr", 13), ("gcn_spgemm_fill_csr", 17)]
U24 = 2.0 ** -24


@pytest.mark.parametrize("name, nargs", SYMBOLS)
def test_new_symbols_exported_and_bound(name, nargs):
    lib = ctypes.CDLL(gcn_amd.LIB_PATH)
    assert hasattr(lib, name) and name in _lib.SIGNATURES
    fn = getattr(gcn_amd.load_library(), name)
    assert fn.restype is ctypes.c_int and fn.argtypes == _lib.SIGNATURES[name][1] and len(fn.argtypes) == nargs
    if name != "gcn_spgemm_ws_bytes":
        assert fn.argtypes[-1] is ctypes.c_void_p      # (void* stream last)
    assert callable(gcn_amd.spgemm) and callable(gcn_amd.hypergraph_laplacian)


def test_limits_of_the_binding_are_the_headers_and_the_workspace_rule_is_the_librarys():
    text = open(os.path.join(ROOT, "include", "gcn_spmm.h")).read()
    for macro, value in (("GCN_SPGEMM_WAVE_MAX", _lib.SPGEMM_WAVE_MAX), ("GCN_SPGEMM_BLOCK_MAX", _lib.SPGEMM_BLOCK_MAX),
                         ("GCN_SPGEMM_DENSE_BLOCKS", _lib.SPGEMM_DENSE_BLOCKS)):
        m = re.search(r"#define\s+" + macro + r"\s+(\d+)\b", text)
        assert m and int(m.group(1)) == value, macro
    assert 64 <= _lib.SPGEMM_WAVE_MAX < _lib.SPGEMM_BLOCK_MAX and _lib.SPGEMM_DENSE_BLOCKS >= 1
    lib = gcn_amd.load_library()
    for m, n in ((0, 0), (1, 1), (5, 7), (4, 0), (6000, 10240), (2 ** 31 - 1, 2 ** 31 - 1)):
        out = ctypes.c_size_t(0)
        assert lib.gcn_spgemm_ws_bytes(m, n, ctypes.byref(out)) == 0
        assert out.value == _lib.spgemm_ws_bytes(m, n) and out.value >= 16 + 4 * m + 8 * n * _lib.SPGEMM_DENSE_BLOCKS
    assert [_lib.spgemm_slots(k) for k in (0, 1, 32, 33, 64, 512, 513, 8192)] == [64, 64, 64, 128, 128, 1024, 2048, 16384]


def _host_ptr():
    buf = (ctypes.c_int32 * 64)()                      # a host array stands in for pointers only looked at, never followed
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def _each(fn, good, changes):
    for i, bad in changes:
        args = list(good)
        args[i] = bad
        assert fn(*args) == INVALID, (i, bad)


def test_bad_arguments_are_rejected_before_any_launch():
    lib = gcn_amd.load_library()
    _keep, p = _host_ptr()
    out = ctypes.c_size_t(0)
    assert lib.gcn_spgemm_ws_bytes(-1, 5, ctypes.byref(out)) == INVALID and lib.gcn_spgemm_ws_bytes(5, -1, ctypes.byref(out)) == INVALID
    assert lib.gcn_spgemm_ws_bytes(5, 5, None) == INVALID
    ws = _lib.spgemm_ws_bytes(5, 7)
    # count(a_rowptr, a_col, m, p, nnz_a, b_rowptr, b_col, n, nnz_b, out_len, ws, ws_bytes, stream)
    good = [p, p, 5, 6, 4, p, p, 7, 3, p, p, ws, None]
    _each(lib.gcn_spgemm_count_csr, good, [(0, None), (1, None), (5, None), (6, None), (9, None), (10, None), (2, -1), (3, -1),
                                           (4, -1), (7, -1), (8, -1), (11, ws - 1), (11, 0)])
    assert lib.gcn_spgemm_count_csr(None, None, 0, 6, 4, None, None, 7, 3, None, None, 0, None) == 0          # no rows
    assert lib.gcn_spgemm_count_csr(None, None, 5, 6, 0, None, None, 7, 3, None, None, 0, None) == INVALID    # ... but out_len
    # fill(a_rowptr, a_col, a_val, m, p, nnz_a, b_rowptr, b_col, b_val, n, nnz_b, out_rowptr, out_col, out_val, ws, ws_bytes, stream)
    good = [p, p, p, 5, 6, 4, p, p, p, 7, 3, p, p, p, p, ws, None]
    _each(lib.gcn_spgemm_fill_csr, good, [(0, None), (1, None), (6, None), (7, None), (11, None), (12, None), (14, None),
                                          (13, None),                           # values in without values out
                                          (3, -1), (4, -1), (5, -1), (9, -1), (10, -1), (15, ws - 1), (15, 0)])
    pattern = list(good)
    pattern[2] = pattern[8] = None                      # both operands patterns: values out are refused
    assert lib.gcn_spgemm_fill_csr(*pattern) == INVALID
    for i in (2, 8):                                    # one pattern operand still has values out
        args = list(good)
        args[i], args[13] = None, None
        assert lib.gcn_spgemm_fill_csr(*args) == INVALID
    assert lib.gcn_spgemm_fill_csr(None, None, None, 0, 6, 4, None, None, None, 7, 3, None, None, None, None, 0, None) == 0
    # no product exists: the fill has nothing to write and needs out_rowptr only
    assert lib.gcn_spgemm_fill_csr(None, None, None, 5, 6, 0, None, None, None, 7, 3, p, None, None, None, 0, None) == 0
    assert lib.gcn_spgemm_fill_csr(None, None, None, 5, 6, 0, None, None, None, 7, 3, None, None, None, None, 0, None) == INVALID


class _FakeAdj(gcn_amd.CsrAdjacency):
    """a CsrAdjacency shell with host arrays (the constructor refuses CPU tensors) and a device of the test's choosing:
    enough to reach the checks that run before any native call"""

    def __init__(self, shape=(3, 3), device="cpu"):
        self.m, self.n, self.nnz = shape[0], shape[1], 4
        self.rowptr = torch.tensor([0, 2, 3, 4], dtype=torch.int32)
        self.col = torch.tensor([0, 1, 2, 0], dtype=torch.int32)
        self.val = torch.ones(4)
        self.device = torch.device(device)
        self.mutable_values = False
        self.symmetric = False
        self.chunk_nnz = 0


def test_spgemm_checks_its_arguments_in_order():
    not_adj = torch.eye(3).to_sparse()
    with pytest.raises(TypeError):
        gcn_amd.spgemm(not_adj, _FakeAdj())
    with pytest.raises(TypeError):                             # (the types of both come before any device)
        gcn_amd.spgemm(_FakeAdj(), not_adj)
    with pytest.raises(gcn_amd.GcnAmdError, match="CPU"):      # the device comes before the shapes
        gcn_amd.spgemm(_FakeAdj((3, 4)), _FakeAdj((3, 3)))
    with pytest.raises(gcn_amd.GcnAmdError, match="CPU"):
        gcn_amd.spgemm(_FakeAdj((3, 4), "cuda:0"), _FakeAdj((3, 3)))
    with pytest.raises(gcn_amd.GcnAmdError, match="one device"):
        gcn_amd.spgemm(_FakeAdj((3, 4), "cuda:0"), _FakeAdj((3, 3), "cuda:1"))
    with pytest.raises(ValueError, match="a.n must equal b.m"):
        gcn_amd.spgemm(_FakeAdj((3, 4), "cuda:0"), _FakeAdj((3, 3), "cuda:0"))
    doc = gcn_amd.spgemm.__doc__
    assert "One host synchronisation" in doc and "two when" in doc and "not capturable" in doc and "not differentiable" in doc


def test_hypergraph_laplacian_checks_its_arguments_in_order():
    with pytest.raises(TypeError):
        gcn_amd.hypergraph_laplacian(torch.eye(3).to_sparse(), edge_weight="bad")
    with pytest.raises(gcn_amd.GcnAmdError, match="CPU"):      # the device of H comes before the weights
        gcn_amd.hypergraph_laplacian(_FakeAdj(), edge_weight="bad")
    H = _FakeAdj((3, 4), "cuda:0")
    for bad in ("ones", 1.0, torch.ones(3), torch.ones(4, dtype=torch.float64), torch.ones(1, 4), [1.0] * 4):
        with pytest.raises(ValueError, match="edge_weight"):
            gcn_amd.hypergraph_laplacian(H, edge_weight=bad)
    with pytest.raises(gcn_amd.GcnAmdError, match="device"):
        gcn_amd.hypergraph_laplacian(H, edge_weight=torch.ones(4))
    assert "Not differentiable" in gcn_amd.hypergraph_laplacian.__doc__ and "not capturable" in gcn_amd.hypergraph_laplacian.__doc__


# ---- the numpy twins -----------------------------------------------------------------------------------------------------------
def _random_csr(m, n, density, rng, repeats=False):
    """positive values in [0.5, 1.5); rows unsorted; with `repeats` some (row, column) pairs are stored twice"""
    A = sp.random(m, n, density=density, format="coo", random_state=rng, data_rvs=lambda k: 0.5 + rng.random(k))
    rows, cols, vals = A.row, A.col, A.data.astype(np.float32)
    if repeats:
        again = rng.random(len(rows)) < 0.2
        rows, cols = np.concatenate([rows, rows[again]]), np.concatenate([cols, cols[again]])
        vals = np.concatenate([vals, (0.5 + rng.random(int(again.sum()))).astype(np.float32)])
    order = rng.permutation(len(rows))
    order = order[np.argsort(rows[order], kind="stable")]
    rp = np.zeros(m + 1, np.int32)
    rp[1:] = np.cumsum(np.bincount(rows, minlength=m))
    return rp, cols[order].astype(np.int32), vals[order]


def summation_bound(a, b, shape_a, shape_b):
    """(the fp64 product, the bound t * 2^-24 * sum |a b| of every entry of its pattern) for (rowptr, col, val) operands: t
    products rounded once each and t - 1 additions, every error at most 2^-24 of a partial sum that sum |a b| bounds.  The
    matrices are built from the arrays as they are: a pair that a stores twice is two products"""
    def mats(x, shape):
        return [sp.csr_matrix((d, x[1], x[0]), shape=shape) for d in (x[2].astype(np.float64), np.abs(x[2]).astype(np.float64),
                                                                       np.ones(len(x[2])))]
    (a64, absa, onea), (b64, absb, oneb) = mats(a, shape_a), mats(b, shape_b)
    assert a64.nnz == len(a[1]) and b64.nnz == len(b[1])
    ref, mag, t = (a64 @ b64).tocsr(), (absa @ absb).tocsr(), (onea @ oneb).tocsr()
    for x in (ref, mag, t):
        x.sort_indices()
    assert np.array_equal(ref.indices, mag.indices) and np.array_equal(ref.indices, t.indices)
    return ref, t.data * U24 * mag.data


def test_twin_is_scipys_product_within_the_summation_bound():
    rng = np.random.default_rng(0)
    a = _random_csr(200, 150, 0.06, rng, repeats=True)  # A may repeat pairs; B holds a column once per row
    b = _random_csr(150, 180, 0.05, rng)
    rp, ci, va, products = spgemm_ref(*a, *b, 150, 180)
    ref, bound = summation_bound(a, b, (200, 150), (150, 180))
    assert np.array_equal(rp, ref.indptr) and np.array_equal(ci, ref.indices) and len(ci) > 5000
    assert np.all(np.diff(ci)[np.diff(np.repeat(np.arange(200), np.diff(rp))) == 0] > 0)          # rows ascend strictly
    err = np.abs(va.astype(np.float64) - ref.data)
    print("largest error / bound", np.max(err / bound))
    assert va.dtype == np.float32 and np.all(err <= bound)
    lens_b = np.diff(b[0])
    assert np.array_equal(products, np.add.reduceat(np.append(lens_b[a[1]], 0), a[0][:-1]) * (np.diff(a[0]) > 0))
    # patterns: the same pattern; a pattern operand counts as ones; two patterns have no values
    assert spgemm_ref(a[0], a[1], None, b[0], b[1], None, 150, 180)[2] is None
    half = spgemm_ref(a[0], a[1], None, *b, 150, 180)
    ones = spgemm_ref(a[0], a[1], np.ones_like(a[2]), *b, 150, 180)
    assert np.array_equal(half[1], ci) and np.array_equal(half[2].view(np.int32), ones[2].view(np.int32))


def test_twin_fold_order_special_values_and_operands_out_of_range():
    f = np.float32
    # row 0: (0, j = 0, 1e8), (0, 1, 1), (0, 2, -1e8), every B row [column 3: 1]: (1e8 + 1) - 1e8 = 0 in fp32, not 1
    a = (np.array([0, 3, 6, 7], np.int32), np.array([0, 1, 2, 1, 0, 2, 0], np.int32), np.array([1e8, 1, -1e8, 1, 1e8, -1e8, -0.0], f))
    b = (np.array([0, 1, 2, 3], np.int32), np.array([3, 3, 3], np.int32), np.ones(3, f))
    rp, ci, va, products = spgemm_ref(*a, *b, 3, 5)
    assert rp.tolist() == [0, 1, 2, 3] and ci.tolist() == [3, 3, 3] and products.tolist() == [3, 3, 1]
    assert va[0] == 0 and va[1] == 0 and np.signbit(va[2]) and va[2] == 0          # 1 + 1e8 - 1e8 = 0 as well; a lone -0.0
    # an A column outside [0, p), a B column outside [0, n), row pointers outside their arrays: nothing, and no product counted
    a = (np.array([0, 2, 9, 3], np.int32), np.array([0, 7, -1], np.int32), np.ones(3, f))
    b = (np.array([0, 2, 5], np.int32), np.array([1, 9], np.int32), np.ones(2, f))
    rp, ci, va, products = spgemm_ref(*a, *b, 2, 5)
    assert rp.tolist() == [0, 1, 1, 1] and ci.tolist() == [1] and products.tolist() == [2, 0, 0]


# ---- the hypergraph Laplacian ---------------------------------------------------------------------------------------------------
def hypergraph_fixture():
    """a 40 x 12 incidence matrix with values in (0, 1] (sixteenths, so every fp64 sum is exact in any order), vertex 17 in
    no hyperedge, some memberships stored twice and rows unsorted -> (rowptr, col, val, dense H fp64, weights)"""
    rng = np.random.default_rng(3)
    n, e = 40, 12
    dense = np.zeros((n, e))
    mask = rng.random((n, e)) < 0.3
    mask[17] = False
    mask[5, :] = False
    mask[5, 4] = True                                   # a vertex in one hyperedge
    dense[mask] = rng.integers(1, 17, int(mask.sum())) / 16
    rows, cols = np.nonzero(dense)
    vals = dense[rows, cols]
    split = rng.random(len(rows)) < 0.25                # stored as two halves (eighths and sixteenths split exactly)
    rows, cols = np.concatenate([rows, rows[split]]), np.concatenate([cols, cols[split]])
    vals = np.concatenate([np.where(split, vals / 2, vals), vals[split] / 2])
    order = rng.permutation(len(rows))
    order = order[np.argsort(rows[order], kind="stable")]
    rp = np.zeros(n + 1, np.int32)
    rp[1:] = np.cumsum(np.bincount(rows, minlength=n))
    w = (rng.integers(1, 9, e) / 4).astype(np.float32)
    return rp, cols[order].astype(np.int32), vals[order].astype(np.float32), dense, w


def dense_g(H, w):
    """hypergraph_utils._generate_G_from_H (variable_weight=False) in fp64, a zero degree giving a zero factor"""
    DV = np.sum(H * w, axis=1)
    DE = np.sum(H, axis=0)
    with np.errstate(divide="ignore"):
        invDE = np.diag(np.where(DE == 0, 0.0, np.power(DE, -1.0)))
        DV2 = np.diag(np.where(DV == 0, 0.0, np.power(DV, -0.5)))
    return DV2 @ H @ np.diag(w) @ invDE @ H.T @ DV2


def shared_hyperedges(H):
    """the largest number of hyperedges two vertices share (the terms of an entry of G)"""
    return int(((H > 0).astype(np.int64) @ (H > 0).astype(np.int64).T).max())


@pytest.mark.parametrize("weighted", [False, True])
def test_twin_laplacian_is_the_dense_formula(weighted):
    rp, ci, va, dense, w = hypergraph_fixture()
    assert len(ci) > int((dense > 0).sum()) and np.array_equal(sorted_merged_ref(rp, ci, va)[2], dense[dense > 0].astype(np.float32))
    grp, gci, gva = hypergraph_laplacian_ref(rp, ci, va, 12, w if weighted else None)
    ref = dense_g(dense, w.astype(np.float64) if weighted else np.ones(12))
    G = sp.csr_matrix((gva, gci, grp), shape=(40, 40))
    assert np.array_equal(G.toarray() != 0, ref != 0) and grp[18] == grp[17] and np.all(ref[17] == 0)
    # every value of L is one rounding to fp32 away from its fp64 value (2^-24 relative; the fp64 arithmetic adds 2^-50) -> a
    # product of two within 3 * 2^-24 with its own rounding, d non-negative terms added with d - 1 roundings: (d + 2) * 2^-24 to
    # first order, (d + 4) * 2^-24 with the higher-order terms and the fp64 noise
    d = shared_hyperedges(dense)
    err = np.abs(G.toarray() - ref)
    print("largest relative error", (err[ref != 0] / ref[ref != 0]).max(), "bound", (d + 4) * U24)
    assert d >= 3 and np.all(err <= (d + 4) * U24 * ref)
    Gt = G.T.tocsr()
    Gt.sort_indices()
    assert np.array_equal(Gt.indptr, grp) and np.array_equal(Gt.indices, gci) and np.array_equal(Gt.data.view(np.int32), gva.view(np.int32))
    trp, tci, tva = transpose_ref(grp, gci, gva, 40)
    assert np.array_equal(trp, grp) and np.array_equal(tci, gci) and np.array_equal(tva.view(np.int32), gva.view(np.int32))

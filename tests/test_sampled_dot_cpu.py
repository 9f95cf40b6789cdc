"""The sampled sparse product without a GPU: the entry point is exported and bound, it refuses bad arguments before anything
is launched, the Python layer checks its arguments in the documented order, and the numpy twin the GPU tests compare with
(tests/sampled_dot_ref.py) agrees with the dense fp64 formula within the summation bound, with spgemm_ref bit for bit on
C's own pattern, and with the dense gradients of the product on the operands' patterns."""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import gcn_amd
from gcn_amd import _lib
from sampled_dot_ref import sampled_dot_ref
from spgemm_ref import spgemm_ref, transpose_ref
from test_spgemm_cpu import INVALID, _FakeAdj, _each, _host_ptr, _random_csr, summation_bound
from util import ROOT

NAME, NARGS = "gcn_csr_sampled_dot_f32", 19


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.int32)


def test_symbol_exported_and_bound():
    lib = ctypes.CDLL(gcn_amd.LIB_PATH)
    assert hasattr(lib, NAME) and NAME in _lib.SIGNATURES
    fn = getattr(gcn_amd.load_library(), NAME)
    assert fn.restype is ctypes.c_int and fn.argtypes == _lib.SIGNATURES[NAME][1] and len(fn.argtypes) == NARGS
    assert fn.argtypes[-1] is ctypes.c_void_p          # (void* stream last)
    text = open(os.path.join(ROOT, "include", "gcn_spmm.h")).read()
    m = re.search(r"#define\s+GCN_SAMPLED_DOT_WS_BYTES\s+(\d+)\b", text)
    assert m and int(m.group(1)) == _lib.SAMPLED_DOT_WS_BYTES
    assert "tests/sampled_dot_ref.py" in text and "meant to be re-implemented" in text
    for f in (gcn_amd.sampled_dot, gcn_amd.SparseProduct, gcn_amd.HypergraphLaplacian, gcn_amd.HGNNConv, gcn_amd.HGNN):
        assert callable(f)
    assert gcn_amd.__version__ == "0.4.0"


def test_bad_arguments_are_rejected_before_any_launch():
    lib = gcn_amd.load_library()
    _keep, p = _host_ptr()
    ws = _lib.SAMPLED_DOT_WS_BYTES
    # (p_rowptr, p_col, mp, np, nnz_p, x_rowptr, x_col, x_val, nnz_x, y_rowptr, y_col, y_val, nnz_y, w, x_by_col, out, ws, ws_bytes, stream)
    good = [p, p, 5, 6, 4, p, p, p, 7, p, p, p, 3, 9, 0, p, p, ws, None]
    _each(lib.gcn_csr_sampled_dot_f32, good, [(0, None), (1, None), (5, None), (6, None), (9, None), (10, None), (15, None),
                                              (16, None), (2, -1), (3, -1), (4, -1), (8, -1), (12, -1), (13, -1), (17, ws - 1),
                                              (17, 0)])
    none = [None, None, 0, 6, 4, None, None, None, 7, None, None, None, 3, 9, 0, None, None, 0, None]
    assert lib.gcn_csr_sampled_dot_f32(*none) == 0                              # no rows: nothing to do, nothing looked at
    none[2], none[4] = 5, 0
    assert lib.gcn_csr_sampled_dot_f32(*none) == 0                              # no entries
    none[3] = -1
    assert lib.gcn_csr_sampled_dot_f32(*none) == INVALID                        # ... but the sizes are still checked


def test_python_layer_checks_its_arguments_in_order():
    not_adj = torch.eye(3).to_sparse()
    cpu, dev0, dev1 = _FakeAdj(), _FakeAdj((3, 3), "cuda:0"), _FakeAdj((3, 3), "cuda:1")
    for args in ((not_adj, cpu, cpu), (cpu, not_adj, cpu), (cpu, cpu, (not_adj, None)), (cpu, (not_adj, torch.ones(4)), cpu)):
        with pytest.raises(TypeError):                         # the types of all three come before any device
            gcn_amd.sampled_dot(*args)
    with pytest.raises(gcn_amd.GcnAmdError, match="CPU"):      # the device comes before the shapes
        gcn_amd.sampled_dot(dev0, _FakeAdj((4, 3), "cuda:0"), cpu)
    with pytest.raises(gcn_amd.GcnAmdError, match="one device"):
        gcn_amd.sampled_dot(dev0, _FakeAdj((4, 3), "cuda:0"), dev1)
    P = _FakeAdj((3, 5), "cuda:0")
    for x, y, by_col in ((_FakeAdj((4, 7), "cuda:0"), _FakeAdj((5, 7), "cuda:0"), False),      # x.m != P.m
                         (_FakeAdj((3, 7), "cuda:0"), _FakeAdj((3, 7), "cuda:0"), False),      # y.m != P.n
                         (_FakeAdj((3, 7), "cuda:0"), _FakeAdj((5, 8), "cuda:0"), False),      # widths differ
                         (_FakeAdj((3, 7), "cuda:0"), _FakeAdj((5, 7), "cuda:0"), True)):      # fits the other mode only
        with pytest.raises(ValueError, match="x_by_col"):
            gcn_amd.sampled_dot(P, x, y, x_by_col=by_col)
    x, y = _FakeAdj((3, 7), "cuda:0"), _FakeAdj((5, 7), "cuda:0")
    for bad in (torch.ones(3), torch.ones(4, dtype=torch.float64), torch.ones(1, 4), [1.0] * 4):
        with pytest.raises(ValueError, match="values"):        # the shapes come before the replacement values
            gcn_amd.sampled_dot(P, (x, bad), y)
    with pytest.raises(gcn_amd.GcnAmdError, match="device"):
        gcn_amd.sampled_dot(P, x, (y, torch.ones(4)))
    doc = gcn_amd.sampled_dot.__doc__
    assert "Not differentiable" in doc and "capturable" in doc and "The checks, in this order" in doc
    # SparseProduct: spgemm's checks, in spgemm's order
    with pytest.raises(TypeError):
        gcn_amd.SparseProduct(not_adj, cpu)
    with pytest.raises(gcn_amd.GcnAmdError, match="CPU"):
        gcn_amd.SparseProduct(_FakeAdj((3, 4)), _FakeAdj((3, 3)))
    with pytest.raises(gcn_amd.GcnAmdError, match="one device"):
        gcn_amd.SparseProduct(_FakeAdj((3, 4), "cuda:0"), _FakeAdj((3, 3), "cuda:1"))
    with pytest.raises(ValueError, match="a.n must equal b.m"):
        gcn_amd.SparseProduct(_FakeAdj((3, 4), "cuda:0"), _FakeAdj((3, 3), "cuda:0"))
    with pytest.raises(TypeError):
        gcn_amd.HypergraphLaplacian(not_adj)
    with pytest.raises(gcn_amd.GcnAmdError, match="CPU"):
        gcn_amd.HypergraphLaplacian(cpu)
    assert "not differentiable" in gcn_amd.spgemm.__doc__ and "SparseProduct" in gcn_amd.spgemm.__doc__
    assert "Not differentiable" in gcn_amd.hypergraph_laplacian.__doc__ and "HypergraphLaplacian" in gcn_amd.hypergraph_laplacian.__doc__


# ---- the numpy twin ------------------------------------------------------------------------------------------------------------
def _sorted(rp, ci, va):
    """the rows column-sorted (the operands here hold a column once per row)"""
    ci, va = ci.copy(), va.copy()
    for i in range(len(rp) - 1):
        o = np.argsort(ci[rp[i]:rp[i + 1]], kind="stable")
        ci[rp[i]:rp[i + 1]], va[rp[i]:rp[i + 1]] = ci[rp[i]:rp[i + 1]][o], va[rp[i]:rp[i + 1]][o]
    return rp, ci, va


def _dense_bound(x, y_t, shape_x, shape_yt):
    """(fp64 x · y_t dense, the summation bound dense — 0 where the product has no term) for CSR triples"""
    ref, bound = summation_bound(x, y_t, shape_x, shape_yt)
    B = sp.csr_matrix((bound, ref.indices, ref.indptr), shape=ref.shape)
    return ref.toarray(), B.toarray()


def _check_on_pattern(got, p, dense, bound):
    rows = np.repeat(np.arange(len(p[0]) - 1), np.diff(p[0]))
    err = np.abs(got.astype(np.float64) - dense[rows, p[1]])
    lim = bound[rows, p[1]]
    print("largest error / bound", np.max(err[lim > 0] / lim[lim > 0]), "entries without a product", int((lim == 0).sum()))
    assert got.dtype == np.float32 and np.all(err <= lim)      # (an entry without a product is exactly 0)


def _operands():
    """A [40 x 30] with repeated pairs and unsorted rows, B [30 x 50] column-sorted with every column once per row"""
    rng = np.random.default_rng(11)
    a = _random_csr(40, 30, 0.3, rng, repeats=True)
    b = _sorted(*_random_csr(30, 50, 0.25, rng))
    return a, b


def test_twin_is_the_dense_formula_within_the_summation_bound():
    rng = np.random.default_rng(5)
    a, b = _operands()
    p = _random_csr(40, 30, 0.4, rng)                       # a pattern of its own: P [40 x 30], X = A [40 x 30], Y [30 x 30]
    y = _sorted(*_random_csr(30, 30, 0.3, rng))
    y_t = transpose_ref(*y, 30)
    dense, bound = _dense_bound(a, y_t, (40, 30), (30, 30))
    got = sampled_dot_ref(p[0], p[1], 30, *a, *y, 30, x_by_col=False)
    assert len(p[1]) > 300
    _check_on_pattern(got, p, dense, bound)
    # x_by_col: the entry (i, j) takes X's row j and Y's row i: (X · Yᵀ)[j, i]
    pt = transpose_ref(p[0], p[1], np.zeros(len(p[1]), np.float32), 30)         # P' [30 x 40]
    got = sampled_dot_ref(pt[0], pt[1], 40, *a, *y, 30, x_by_col=True)
    _check_on_pattern(got, pt, dense.T, bound.T)
    # patterns count as ones
    ones = sampled_dot_ref(p[0], p[1], 30, a[0], a[1], None, y[0], y[1], None, 30)
    common = (sp.csr_matrix((np.ones(len(a[1])), a[1], a[0]), shape=(40, 30)) @ sp.csr_matrix((np.ones(len(y[1])), y[1], y[0]),
                                                                                             shape=(30, 30)).T).toarray()
    rows = np.repeat(np.arange(40), np.diff(p[0]))
    assert np.array_equal(ones, common[rows, p[1]].astype(np.float32)) and ones.max() >= 2


def test_twin_on_the_products_own_pattern_is_spgemm_ref_bit_for_bit():
    a, b = _operands()
    assert len(a[1]) > len(set(zip(np.repeat(np.arange(40), np.diff(a[0])).tolist(), a[1].tolist())))          # A repeats pairs
    assert any(np.any(np.diff(a[1][a[0][i]:a[0][i + 1]]) < 0) for i in range(40))                              # ... unsorted
    rp, ci, va, _ = spgemm_ref(*a, *b, 30, 50)
    bt = transpose_ref(*b, 50)
    got = sampled_dot_ref(rp, ci, 50, *a, *bt, 30)
    print("entries", len(ci))
    assert len(ci) > 600 and np.array_equal(bits(got), bits(va))


def test_twin_gradients_are_the_dense_gradients_on_the_patterns():
    rng = np.random.default_rng(7)
    a, b = _operands()
    rp, ci, va, _ = spgemm_ref(*a, *b, 30, 50)
    g = (0.5 + rng.random(len(ci))).astype(np.float32)
    c = (rp, ci, g)
    # grad_a on A's pattern: P = A, X = B, Y = (C, g), x_by_col -> (Gd · Bdᵀ)[i, j]; the terms are B's entries of row j
    ga = sampled_dot_ref(a[0], a[1], 30, *b, *c, 50, x_by_col=True)
    dense, bound = _dense_bound(b, transpose_ref(*c, 50), (30, 50), (50, 40))   # B · Gᵀ [30 x 40]
    _check_on_pattern(ga, a, dense.T, bound.T)
    # grad_b on B's pattern: P = B, X = Aᵀ, Y = (Cᵀ, g) -> (Adᵀ · Gd)[j, c]
    at, ct = transpose_ref(*a, 30), transpose_ref(*c, 50)
    gb = sampled_dot_ref(b[0], b[1], 50, *at, *ct, 40)
    dense, bound = _dense_bound(at, c, (30, 40), (40, 50))                      # Aᵀ · G [30 x 50]
    _check_on_pattern(gb, b, dense, bound)


def test_twin_fold_order_special_values_and_operands_out_of_range():
    f = np.float32
    big = f(2.0 ** 24)
    # X row 0: 2^24, 1, -2^24 on columns 0, 1, 2; Y row 0 holds all three with ones: (2^24 + 1) - 2^24 = 0 in fp32, not 1
    x = (np.array([0, 3, 6, 7, 7], np.int32), np.array([0, 1, 2, 1, 0, 2, 4, ], np.int32), np.array([big, 1, -big, 1, big, -big, -0.0], f))
    y = (np.array([0, 5, 5], np.int32), np.array([0, 1, 2, 4, 6], np.int32), np.ones(5, f))
    p = (np.array([0, 2, 3, 5, 6], np.int32), np.array([0, 1, 0, 0, 7, 0], np.int32))
    out = sampled_dot_ref(p[0], p[1], 2, *x, *y, 7)
    assert out[0] == 0 and not np.signbit(out[0])            # the fold order
    assert bits(out[1:2])[0] == 0                            # Y's row 1 is empty: +0.0
    assert out[2] == 0                                       # 1 + 2^24 - 2^24
    assert np.signbit(out[3]) and out[3] == 0                # a lone -0.0 stays -0.0
    assert bits(out[4:5])[0] == 0                            # a P column out of range: +0.0
    assert bits(out[5:6])[0] == 0                            # X's row 3 is empty
    # an X column outside [0, w) contributes nothing; unusable row pointers: an empty operand row, an unwritten P row
    x = (np.array([0, 3, 9], np.int32), np.array([0, 9, -1], np.int32), np.ones(3, f))
    y = (np.array([0, 2, 1], np.int32), np.array([0, 9], np.int32), np.ones(2, f))
    p = (np.array([0, 2, 1], np.int32), np.array([0, 1], np.int32))
    out = sampled_dot_ref(p[0], p[1], 2, *x, *y, 5, out=np.full(2, 7, f))
    assert out.tolist() == [1.0, 0.0]                        # (0, 0): column 0 only; (0, 1): Y's row 1 descends -> empty
    out = sampled_dot_ref(p[0], p[1], 2, *x, *y, 5, x_by_col=True, out=np.full(2, 7, f))
    assert out.tolist() == [1.0, 0.0]                        # (0, 1) -> X's row 1 is unusable
    p = (np.array([0, 3, 2], np.int32), np.array([0, 1], np.int32))
    out = sampled_dot_ref(p[0], p[1], 2, *x, *y, 5, out=np.full(2, 7, f))
    assert out.tolist() == [7.0, 7.0]                        # both P rows unusable (3 > nnz; descending): nothing written

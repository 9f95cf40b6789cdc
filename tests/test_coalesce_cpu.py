"""The device merge without a GPU: the four entry points are exported and bound and refuse bad arguments before anything is
launched, the codes of the binding are the header's, the Python layer checks its arguments in the documented order, and
the numpy twins the GPU tests compare with (tests/coalesce_ref.py) agree with scipy, and with the project's own host
pipeline, on a fixture with repeated pairs, existing and missing diagonals and empty rows."""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import gcn_amd
from gcn_amd import _lib
from gcn_amd.preprocess import normalize_adj
from coalesce_ref import (coalesce_ref, degree_ref, gcn_adjacency_ref, normalize_ref, sorted_csr_ref, symmetrize_ref,
                          within_one_ulp)
from util import ROOT

INVALID = 1                                            # GCN_ERR_INVALID_ARG
SYMBOLS = [("gcn_csr_coalesce_count", 10), ("gcn_csr_coalesce_fill", 17), ("gcn_csr_degree_f64", 6), ("gcn_csr_normalize_f32", 10)]


def _host_ptr():
    buf = (ctypes.c_int32 * 64)()                      # a host array stands in for pointers only looked at, never followed
    return buf, ctypes.cast(buf, ctypes.c_void_p)


@pytest.mark.parametrize("name, nargs", SYMBOLS)
def test_new_symbols_exported_and_bound(name, nargs):
    lib = ctypes.CDLL(gcn_amd.LIB_PATH)
    assert hasattr(lib, name) and name in _lib.SIGNATURES
    fn = getattr(gcn_amd.load_library(), name)
    assert fn.restype is ctypes.c_int and fn.argtypes == _lib.SIGNATURES[name][1] and len(fn.argtypes) == nargs
    assert fn.argtypes[-1] is ctypes.c_void_p          # (void* stream last)
    for fn_name in ("coalesce_csr", "symmetrize", "normalize_csr", "gcn_adjacency"):
        assert callable(getattr(gcn_amd, fn_name))


def test_codes_of_the_binding_are_the_headers():
    text = open(os.path.join(ROOT, "include", "gcn_spmm.h")).read()
    for macro, value in (("GCN_COALESCE_WS_BYTES", _lib.COALESCE_WS_BYTES), ("GCN_COALESCE_SUM", _lib.COALESCE_SUM),
                         ("GCN_COALESCE_MAX", _lib.COALESCE_MAX), ("GCN_COALESCE_MIN", _lib.COALESCE_MIN),
                         ("GCN_COALESCE_FIRST", _lib.COALESCE_FIRST), ("GCN_DIAG_KEEP", _lib.DIAG_KEEP),
                         ("GCN_DIAG_DROP", _lib.DIAG_DROP), ("GCN_DIAG_FILL", _lib.DIAG_FILL), ("GCN_DIAG_ADD", _lib.DIAG_ADD),
                         ("GCN_NORM_SYM", _lib.NORM_SYM), ("GCN_NORM_ROW", _lib.NORM_ROW)):
        m = re.search(r"#define\s+" + macro + r"\s+(\d+)\b", text)
        assert m and int(m.group(1)) == value, macro
    assert len({_lib.COALESCE_SUM, _lib.COALESCE_MAX, _lib.COALESCE_MIN, _lib.COALESCE_FIRST}) == 4
    assert len({_lib.DIAG_KEEP, _lib.DIAG_DROP, _lib.DIAG_FILL, _lib.DIAG_ADD}) == 4 and _lib.NORM_SYM != _lib.NORM_ROW


def _each(fn, good, changes):
    for i, bad in changes:
        args = list(good)
        args[i] = bad
        assert fn(*args) == INVALID, (i, bad)


def test_bad_arguments_are_rejected_before_any_launch():
    lib = gcn_amd.load_library()
    _keep, p = _host_ptr()
    ws = _lib.COALESCE_WS_BYTES
    # count(rowptr, col, m, n, nnz, diagonal, out_len, ws, ws_bytes, stream)
    good = [p, p, 5, 5, 4, _lib.DIAG_KEEP, p, p, ws, None]
    _each(lib.gcn_csr_coalesce_count, good, [(0, None), (1, None), (6, None), (7, None), (2, -1), (3, -1), (4, -1), (5, -1),
                                             (5, 4), (8, ws - 1)])
    assert lib.gcn_csr_coalesce_count(None, None, 0, 5, 0, _lib.DIAG_FILL, None, None, 0, None) == 0          # no rows
    # fill(rowptr, col, val, m, n, nnz, reduce, diagonal, diag_value, out_rowptr, out_col, out_val, out_first, seg, ws, ws_bytes, stream)
    good = [p, p, p, 5, 5, 4, _lib.COALESCE_SUM, _lib.DIAG_KEEP, 1.0, p, p, p, p, p, p, ws, None]
    _each(lib.gcn_csr_coalesce_fill, good, [(0, None), (1, None), (9, None), (10, None), (14, None),
                                            (2, None), (11, None),               # values in without values out, and the reverse
                                            (3, -1), (4, -1), (5, -1), (6, -1), (6, 4), (7, -1), (7, 4), (15, ws - 1)])
    assert lib.gcn_csr_coalesce_fill(None, None, None, 0, 5, 0, 0, 0, 1.0, None, None, None, None, None, None, 0, None) == 0
    # degree(rowptr, val, m, nnz, deg, stream)
    good = [p, p, 5, 4, p, None]
    _each(lib.gcn_csr_degree_f64, good, [(0, None), (4, None), (2, -1), (3, -1)])
    assert lib.gcn_csr_degree_f64(None, None, 0, 0, None, None) == 0
    # normalize(rowptr, col, val, m, n, nnz, deg, mode, out_val, stream)
    good = [p, p, p, 5, 5, 4, p, _lib.NORM_SYM, p, None]
    _each(lib.gcn_csr_normalize_f32, good, [(0, None), (1, None), (6, None), (8, None), (3, -1), (4, -1), (5, -1), (7, -1), (7, 2),
                                            (4, 6)])                             # (GCN_NORM_SYM on a 5 x 6 matrix)
    assert lib.gcn_csr_normalize_f32(None, None, None, 5, 5, 0, None, _lib.NORM_ROW, None, None) == 0         # no entries
    assert lib.gcn_csr_normalize_f32(None, None, None, 0, 0, 0, None, _lib.NORM_SYM, None, None) == 0


class _FakeAdj(gcn_amd.CsrAdjacency):
    """a CsrAdjacency shell with host arrays (the constructor refuses CPU tensors): enough to reach the checks that run
    before any native call"""

    def __init__(self, shape=(3, 3)):
        self.m, self.n, self.nnz = shape[0], shape[1], 4
        self.rowptr = torch.tensor([0, 2, 3, 4], dtype=torch.int32)
        self.col = torch.tensor([0, 1, 2, 0], dtype=torch.int32)
        self.val = torch.ones(4)
        self.device = torch.device("cpu")
        self.mutable_values = False
        self.symmetric = False
        self.chunk_nnz = 0


def test_coalesce_csr_checks_its_arguments_in_order():
    not_adj = torch.eye(3).to_sparse()
    for bad in ("mean", None, 0):
        with pytest.raises(ValueError, match="reduce"):        # the options come before the adjacency
            gcn_amd.coalesce_csr(not_adj, reduce=bad)
    for bad in ("zero", None, 2):
        with pytest.raises(ValueError, match="diagonal"):
            gcn_amd.coalesce_csr(not_adj, diagonal=bad)
    for bad in ("1", None, True):
        with pytest.raises(ValueError, match="diag_value"):
            gcn_amd.coalesce_csr(not_adj, diag_value=bad)
    with pytest.raises(TypeError):
        gcn_amd.coalesce_csr(not_adj)
    with pytest.raises(gcn_amd.GcnAmdError, match="CPU"):
        gcn_amd.coalesce_csr(_FakeAdj())
    doc = gcn_amd.coalesce_csr.__doc__
    assert "One host synchronisation" in doc and "not capturable" in doc


def test_symmetrize_and_normalize_csr_check_their_arguments_in_order():
    not_adj = torch.eye(3).to_sparse()
    for bad in ("first", "mean", None):
        with pytest.raises(ValueError, match="reduce"):
            gcn_amd.symmetrize(not_adj, reduce=bad)
    with pytest.raises(TypeError):
        gcn_amd.symmetrize(not_adj)
    with pytest.raises(gcn_amd.GcnAmdError, match="CPU"):      # (the device comes before the shape)
        gcn_amd.symmetrize(_FakeAdj((3, 4)))
    for bad in ("col", None, 1):
        with pytest.raises(ValueError, match="norm"):
            gcn_amd.normalize_csr(not_adj, norm=bad)
    with pytest.raises(TypeError):
        gcn_amd.normalize_csr(not_adj)
    with pytest.raises(gcn_amd.GcnAmdError, match="CPU"):
        gcn_amd.normalize_csr(_FakeAdj())


BAD_IDS = (torch.tensor([0.0, 1.0]), torch.tensor([[0, 1]]), torch.tensor(1), [0, 1], torch.tensor([0, 1], dtype=torch.int16))


def test_gcn_adjacency_checks_its_arguments_in_order():
    r, c = torch.tensor([0, 1], dtype=torch.int64), torch.tensor([1, 0], dtype=torch.int32)
    for bad in BAD_IDS:
        with pytest.raises(ValueError, match="rows"):
            gcn_amd.gcn_adjacency(bad, c, 2)
        with pytest.raises(ValueError, match="cols"):
            gcn_amd.gcn_adjacency(r, bad, 2)
    with pytest.raises(ValueError, match="same length"):
        gcn_amd.gcn_adjacency(r, c[:1], 2)
    for bad in (-1, 1.5, None, True, 2 ** 31):
        with pytest.raises(ValueError, match="n must be"):
            gcn_amd.gcn_adjacency(r, c, bad)
    for bad in ("gcn", torch.ones(3), torch.ones(2, dtype=torch.float64), torch.ones(1, 2), 1.0):
        with pytest.raises(ValueError, match="values"):
            gcn_amd.gcn_adjacency(r, c, 2, values=bad)
    for bad in ("first", "mean", None):
        with pytest.raises(ValueError, match="reduce"):
            gcn_amd.gcn_adjacency(r, c, 2, reduce=bad)
    for bad in ("yes", None, True):
        with pytest.raises(ValueError, match="self_loops"):
            gcn_amd.gcn_adjacency(r, c, 2, self_loops=bad)
    for bad in ("col", 1):
        with pytest.raises(ValueError, match="norm"):
            gcn_amd.gcn_adjacency(r, c, 2, norm=bad)
    for values in (None, torch.ones(2)):
        with pytest.raises(gcn_amd.GcnAmdError, match="CPU"):
            gcn_amd.gcn_adjacency(r, c, 2, values=values)
    assert "NOT DIFFERENTIABLE" in gcn_amd.gcn_adjacency.__doc__


# ---- the numpy twins -----------------------------------------------------------------------------------------------------------
N = 40


def _fixture():
    """a directed 40-vertex edge list in random order with repeated pairs, self-loops on some vertices (not on vertex 0)
    and vertices without any edge; values are small positive multiples of 1/8 (sums are exact in any order)"""
    rng = np.random.default_rng(0)
    rows, cols = rng.integers(0, N, 150), rng.integers(0, N, 150)
    keep = ~np.isin(rows, [7, 23, 39]) & ~np.isin(cols, [7, 23, 39]) & ~((rows == 0) & (cols == 0))
    rows, cols = rows[keep], cols[keep]
    rows = np.concatenate([rows, rows[:25], [5, 5, 11, 30]])           # repeats, and self-loops (one of them twice)
    cols = np.concatenate([cols, cols[:25], [5, 5, 11, 30]])
    vals = (rng.integers(1, 9, len(rows)) / 8).astype(np.float32)
    pairs = rows * N + cols
    assert len(np.unique(pairs)) < len(pairs) - 20 and not np.any((rows == 0) & (cols == 0))
    rp, eid = sorted_csr_ref(rows, cols, N)
    assert (np.diff(rp) == 0).sum() >= 3
    return rows, cols, vals, rp, cols[eid].astype(np.int32), vals[eid]


def _same(got, want):
    """a twin's (rowptr, col, val) against a scipy matrix"""
    want = want.tocsr()
    want.sort_indices()
    return (np.array_equal(got[0], want.indptr) and np.array_equal(got[1], want.indices)
            and np.array_equal(got[2], want.data.astype(np.float32)))


def test_twin_sum_is_scipys_sum_duplicates_and_seg_and_first_describe_the_merge():
    _, _, _, rp, ci, va = _fixture()
    orp, oci, ova, first, seg = coalesce_ref(rp, ci, va, N, "sum")
    A = sp.csr_matrix((va.copy(), ci.copy(), rp.copy()), shape=(N, N))
    A.sum_duplicates()
    assert A.nnz < len(ci) and _same((orp, oci, ova), A)
    assert np.array_equal(oci[seg], ci) and np.all(np.diff(seg) >= 0) and np.array_equal(np.unique(seg), np.arange(len(oci)))
    assert np.array_equal(first, np.flatnonzero(np.diff(seg, prepend=-1)))                 # the head of every run
    assert np.array_equal(coalesce_ref(rp, ci, va, N, "first")[2], va[first])
    pat = coalesce_ref(rp, ci, None, N, "sum")
    assert pat[2] is None and np.array_equal(pat[1], oci) and np.array_equal(pat[4], seg)


def test_twin_max_after_mirroring_is_scipys_maximum_with_the_transpose():
    _, _, _, rp, ci, va = _fixture()
    orp, oci, ova, _, _ = coalesce_ref(rp, ci, va, N, "sum")
    A = sp.csr_matrix((ova, oci, orp), shape=(N, N))
    assert _same(symmetrize_ref(orp, oci, ova, "max"), A.maximum(A.T))
    plus = (A + A.T).tolil()
    plus.setdiag(A.diagonal())                              # (a diagonal entry is not mirrored)
    assert _same(symmetrize_ref(orp, oci, ova, "sum"), plus)
    dense = A.toarray()                                     # min: of the two where both directions are stored, else the one
    both = (dense > 0) & (dense.T > 0)
    assert _same(symmetrize_ref(orp, oci, ova, "min"),
                 sp.csr_matrix(np.where(both, np.minimum(dense, dense.T), np.maximum(dense, dense.T))))


def test_twin_diagonal_codes_are_the_scipy_expressions():
    _, _, _, rp, ci, va = _fixture()
    A = sp.csr_matrix((va.copy(), ci.copy(), rp.copy()), shape=(N, N))
    A.sum_duplicates()
    has = A.diagonal() != 0
    assert has.sum() >= 3 and (~has).sum() >= 3
    D = A.tolil()
    D.setdiag(0)
    D = D.tocsr()
    D.eliminate_zeros()
    got = coalesce_ref(rp, ci, va, N, "sum", "drop")
    assert _same(got[:3], D) and np.all((got[4] == -1) == (ci == np.repeat(np.arange(N), np.diff(rp))))
    dv = 0.375
    got = coalesce_ref(rp, ci, va, N, "sum", "fill", dv)
    assert _same(got[:3], A + sp.diags(np.where(has, 0.0, dv))) and (got[3] == -1).sum() == (~has).sum()
    got = coalesce_ref(rp, ci, va, N, "sum", "add", dv)
    assert _same(got[:3], A + dv * sp.eye(N))
    wide = coalesce_ref(rp, ci, va, N + 5, "sum", "fill", dv)               # the same rows of a 40 x 45 matrix: r < n for all
    assert np.array_equal(wide[0], got[0])
    tall = coalesce_ref(rp, np.minimum(ci, 9), va, 10, "sum", "fill", dv)   # 40 x 10: the rows r >= 10 get no diagonal
    assert (tall[3] == -1).sum() <= 10 and np.all(tall[1] < 10)


def _host_pipeline(rows, cols):
    """the symmetrisation lines of io.load_deeprobust_npz followed by preprocess.normalize_adj, in fp64"""
    adj = sp.coo_matrix((np.ones(len(rows)), (rows, cols)), shape=(N, N)).tocsr()
    adj = (adj + adj.T).tolil()
    adj[adj > 1] = 1
    adj.setdiag(0)
    adj = adj.astype(np.float32).tocsr()
    adj.eliminate_zeros()
    assert adj[0, 0] == 0                                  # (normalize_adj adds the identity only then)
    out = sp.csr_matrix(normalize_adj(adj))
    out.sort_indices()
    return out


def test_twin_pipeline_with_the_defaults_is_the_host_pipeline():
    rows, cols, _, _, _, _ = _fixture()
    host = _host_pipeline(rows, cols)
    orp, oci, ova = gcn_adjacency_ref(rows, cols, N)
    assert np.array_equal(orp, host.indptr) and np.array_equal(oci, host.indices)
    assert ova.dtype == np.float32 and np.all(within_one_ulp(ova, host.data))
    empty = np.flatnonzero(np.diff(orp) == 1)              # a vertex without edges keeps its self-loop alone, weight 1
    assert len(empty) >= 3 and np.all(ova[orp[empty]] == 1)


def test_twin_degree_and_normalize():
    _, _, _, rp, ci, va = _fixture()
    deg = degree_ref(rp, va)
    A = sp.csr_matrix((va.astype(np.float64), ci.copy(), rp.copy()), shape=(N, N))
    assert np.array_equal(deg, np.asarray(A.sum(1)).ravel()) and np.array_equal(degree_ref(rp, None), np.diff(rp))
    row = normalize_ref(rp, ci, va, deg, "row")
    sums = np.add.reduceat(np.append(row, 0), rp[:-1])[np.diff(rp) > 0]
    assert np.allclose(sums, 1, rtol=1e-14, atol=0)
    sym = normalize_ref(rp, ci, va, deg, "sym")            # columns of vertices without edges of their own: scaled by zero
    assert np.all(np.isfinite(sym)) and np.all(sym[deg[ci] == 0] == 0) and np.any(deg == 0)

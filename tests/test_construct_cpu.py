"""Device CSR construction without a GPU: the three entry points are exported and bound and refuse bad arguments before
anything is launched, the workspace rule of the binding is the library's, the Python layer checks its arguments in the
documented order, and the numpy twins the GPU tests compare with (tests/construct_ref.py) agree with scipy on a fixture
with repeated entries and empty rows."""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import gcn_amd
from gcn_amd import _lib
from construct_ref import bucket_ref, csr_from_edges_ref, transpose_ref
from util import ROOT, random_rows_csr

INVALID = 1                                            # GCN_ERR_INVALID_ARG


def _host_ptr():
    buf = (ctypes.c_int32 * 64)()                      # a host array stands in for pointers only looked at, never followed
    return buf, ctypes.cast(buf, ctypes.c_void_p)


@pytest.mark.parametrize("name, nargs", [("gcn_bucket_count_i32", 5), ("gcn_bucket_fill_i32", 8), ("gcn_csr_transpose_gather", 8)])
def test_new_symbols_exported_and_bound(name, nargs):
    lib = ctypes.CDLL(gcn_amd.LIB_PATH)
    assert hasattr(lib, name) and name in _lib.SIGNATURES
    fn = getattr(gcn_amd.load_library(), name)
    assert fn.restype is ctypes.c_int and fn.argtypes == _lib.SIGNATURES[name][1] and len(fn.argtypes) == nargs
    assert fn.argtypes[-1] is ctypes.c_void_p          # (void* stream last)
    text = open(os.path.join(ROOT, "include", "gcn_spmm.h")).read()
    for macro, value in (("GCN_BUCKET_WAVE_MAX", _lib.BUCKET_WAVE_MAX), ("GCN_BUCKET_BLOCK_MAX", _lib.BUCKET_BLOCK_MAX)):
        m = re.search(r"#define\s+" + macro + r"\s+(\d+)\b", text)
        assert m and int(m.group(1)) == value
    assert 64 <= _lib.BUCKET_WAVE_MAX < _lib.BUCKET_BLOCK_MAX
    for fn_name in ("bucket_by_key", "transpose_csr", "csr_from_edges"):
        assert callable(getattr(gcn_amd, fn_name))


def test_bad_arguments_are_rejected_and_empty_problems_launch_nothing():
    lib = gcn_amd.load_library()
    _keep, p = _host_ptr()
    count, fill, gather = lib.gcn_bucket_count_i32, lib.gcn_bucket_fill_i32, lib.gcn_csr_transpose_gather
    for args in ([None, 5, 3, p, None], [p, 5, 3, None, None], [p, -1, 3, p, None], [p, 5, -1, p, None],
                 [None, 0, 3, None, None], [None, 5, 0, None, None]):        # (offsets are written even for an empty problem)
        assert count(*args) == INVALID, args
    big = 1 << 20
    good = [p, 5, 3, p, p, p, big, None]
    for i in (0, 3, 4, 5):                             # each pointer in turn
        args = list(good)
        args[i] = None
        assert fill(*args) == INVALID, i
    for i, bad in ((1, -1), (2, -1)):
        args = list(good)
        args[i] = bad
        assert fill(*args) == INVALID, i
    assert fill(None, 0, 3, None, None, None, 0, None) == 0                   # no keys
    assert fill(None, 5, 0, None, None, None, 0, None) == 0                   # no buckets
    good = [p, 3, 4, p, p, p, p, None]
    for i in (0, 3, 5):
        args = list(good)
        args[i] = None
        assert gather(*args) == INVALID, i
    for i in (4, 6):                                   # values in without values out, and the reverse
        args = list(good)
        args[i] = None
        assert gather(*args) == INVALID, i
    for i in (1, 2):
        args = list(good)
        args[i] = -1
        assert gather(*args) == INVALID, i
    assert gather(p, 0, 4, p, None, p, None, None) == INVALID                 # entries without rows
    assert gather(None, 3, 0, None, None, None, None, None) == 0              # no entries


@pytest.mark.parametrize("count, nbuckets", [(1, 1), (5, 3), (2, 100000), (50, 100000), (300000, 7), (300000, 300000),
                                             (2 ** 31 - 1, 2 ** 31 - 1)])
def test_workspace_rule_of_the_binding_is_the_librarys(count, nbuckets):
    """the fill refuses a workspace one byte short of _lib.bucket_ws_bytes (that it accepts one of exactly that size is what
    every call of the GPU tests shows), and the rule is the one written out in include/gcn_spmm.h"""
    fill = gcn_amd.load_library().gcn_bucket_fill_i32
    _keep, p = _host_ptr()
    need = _lib.bucket_ws_bytes(count, nbuckets)
    assert need % 16 == 0 and need >= 16 + 4 * nbuckets
    assert fill(p, count, nbuckets, p, p, p, need - 1, None) == INVALID
    wave, block = _lib.BUCKET_WAVE_MAX, _lib.BUCKET_BLOCK_MAX
    lists = min(nbuckets, count // 2) + min(nbuckets, count // (wave + 1)) + min(nbuckets, count // (block + 1))
    assert need == (4 * (4 + nbuckets + lists) + 15) // 16 * 16


class _FakeAdj(gcn_amd.CsrAdjacency):
    """a CsrAdjacency shell with host arrays (the constructor refuses CPU tensors): enough to reach the checks that run
    before any native call"""

    def __init__(self):
        self.m, self.n, self.nnz = 3, 3, 4
        self.rowptr = torch.tensor([0, 2, 3, 4], dtype=torch.int32)
        self.col = torch.tensor([0, 1, 2, 0], dtype=torch.int32)
        self.val = torch.ones(4)
        self.device = torch.device("cpu")
        self.mutable_values = False
        self.symmetric = False
        self.chunk_nnz = 0


BAD_IDS = (torch.tensor([0.0, 1.0]), torch.tensor([[0, 1]]), torch.tensor(1), [0, 1], torch.tensor([0, 1], dtype=torch.int16))


def test_bucket_by_key_checks_its_arguments_in_order():
    keys = torch.tensor([0, 1], dtype=torch.int32)
    for bad in (-1, 1.5, None, True, 2 ** 31):
        with pytest.raises(ValueError, match="nbuckets"):
            gcn_amd.bucket_by_key(keys, bad)
    for bad in BAD_IDS:
        with pytest.raises(ValueError, match="keys"):     # dtype and shape come before the device
            gcn_amd.bucket_by_key(bad, 4)
    for dt in (torch.int32, torch.int64):
        with pytest.raises(gcn_amd.GcnAmdError, match="CPU"):
            gcn_amd.bucket_by_key(keys.to(dt), 4)


def test_transpose_csr_checks_its_arguments():
    with pytest.raises(TypeError):
        gcn_amd.transpose_csr(torch.eye(3).to_sparse())
    with pytest.raises(gcn_amd.GcnAmdError, match="CPU"):
        gcn_amd.transpose_csr(_FakeAdj())
    assert "separate" in gcn_amd.transpose_csr.__doc__


def test_csr_from_edges_checks_its_arguments_in_order():
    r, c = torch.tensor([0, 1], dtype=torch.int64), torch.tensor([1, 0], dtype=torch.int32)
    for bad in BAD_IDS:
        with pytest.raises(ValueError, match="rows"):
            gcn_amd.csr_from_edges(bad, c, (2, 2))
        with pytest.raises(ValueError, match="cols"):
            gcn_amd.csr_from_edges(r, bad, (2, 2))
    with pytest.raises(ValueError, match="same length"):
        gcn_amd.csr_from_edges(r, c[:1], (2, 2))
    for bad in (2, (2,), (2, 2, 2), None):
        with pytest.raises(ValueError, match="shape"):
            gcn_amd.csr_from_edges(r, c, bad)
    for bad in ((-1, 2), (2, 1.5), (2 ** 31, 2), (True, 2)):
        with pytest.raises(ValueError, match="shape"):
            gcn_amd.csr_from_edges(r, c, bad)
    for bad in ("sym", torch.ones(3), torch.ones(2, dtype=torch.float64), torch.ones(1, 2), 1.0):
        with pytest.raises(ValueError, match="values"):
            gcn_amd.csr_from_edges(r, c, (2, 2), values=bad)
    with pytest.raises(ValueError, match="square"):
        gcn_amd.csr_from_edges(r, c, (2, 3), values="gcn")
    for values in (None, torch.ones(2), "gcn"):
        with pytest.raises(gcn_amd.GcnAmdError, match="CPU"):
            gcn_amd.csr_from_edges(r, c, (2, 2), values=values)
    doc = gcn_amd.csr_from_edges.__doc__
    assert "NOT MERGED" in doc and "self-loops" in doc and "out of scope" in doc


# ---- the numpy twins ---------------------------------------------------------------------------------------------------------
def _fixture():
    """a 40 x 23 pattern with empty rows, empty columns and repeated (row, column) pairs, values = entry index + 1"""
    lens = np.random.default_rng(0).integers(0, 9, 40)
    lens[[0, 7, 39]] = 0
    rp, ci = random_rows_csr(40, 20, lens, seed=1)     # columns 20 .. 22 stay empty
    rows = np.repeat(np.arange(40), np.diff(rp))
    pairs = rows.astype(np.int64) * 23 + ci
    assert len(np.unique(pairs)) < len(pairs) and (np.diff(rp) == 0).sum() >= 3
    return rp, ci, np.arange(1, len(ci) + 1, dtype=np.float32), rows


def test_twin_bucket_is_a_stable_argsort_with_bincount_offsets():
    keys = np.random.default_rng(2).integers(0, 11, 500)
    keys[keys == 4] = 5                                # an empty bucket
    offsets, perm = bucket_ref(keys, 13)
    assert offsets.dtype == np.int32 and perm.dtype == np.int32 and offsets[0] == 0 and offsets[-1] == 500
    assert np.array_equal(np.sort(perm), np.arange(500))
    for b in range(13):
        seg = perm[offsets[b]:offsets[b + 1]]
        assert np.array_equal(seg, np.flatnonzero(keys == b))             # exactly the bucket's indices, ascending
    offsets, perm = bucket_ref(np.zeros(0, np.int64), 3)
    assert np.array_equal(offsets, [0, 0, 0, 0]) and len(perm) == 0


def test_twin_transpose_is_scipys_with_repeated_entries_kept_apart():
    rp, ci, va, rows = _fixture()
    trp, trow, tval, eid = transpose_ref(rp, ci, va, 23)
    T = sp.csr_matrix((va.astype(np.float64), ci, rp), shape=(40, 23)).T.tocsr()   # (scipy's transpose keeps duplicates too)
    assert T.nnz == len(ci) and np.array_equal(trp, T.indptr)
    assert np.array_equal(rows[eid], trow) and np.array_equal(va[eid], tval)
    for c in range(23):
        seg = slice(trp[c], trp[c + 1])
        assert np.all(ci[eid[seg]] == c) and np.all(np.diff(eid[seg]) > 0)    # source order: rows ascend, repeats in order
        assert np.all(np.diff(trow[seg]) >= 0)
    A = sp.csr_matrix((va.astype(np.float64), ci, rp), shape=(40, 23))
    A.sum_duplicates()
    Tm = sp.csr_matrix((tval.astype(np.float64), trow.copy(), trp.copy()), shape=(23, 40))
    Tm.sum_duplicates()
    assert (abs(Tm - A.T.tocsr())).nnz == 0                                  # the same matrix


def test_twin_csr_from_edges_is_scipys_coo_to_csr():
    rp, ci, va, rows = _fixture()
    order = np.random.default_rng(3).permutation(len(ci))                    # the edges in a random order
    er, ec, ev = rows[order], ci[order], va[order]
    for sort_columns in (True, False):
        frp, fci, fva, eid = csr_from_edges_ref(er, ec, (40, 23), ev, sort_columns)
        assert np.array_equal(frp, rp) and np.array_equal(er[eid], rows) and np.array_equal(ec[eid], fci)
        assert np.array_equal(ev[eid], fva)
        S = sp.coo_matrix((ev.astype(np.float64), (er, ec)), shape=(40, 23)).tocsr()     # (sums the repeated pairs)
        M = sp.csr_matrix((fva.astype(np.float64), fci.copy(), frp.copy()), shape=(40, 23))   # (scipy merges in place)
        M.sum_duplicates()
        assert np.array_equal(S.indptr, M.indptr) and (abs(S - M)).nnz == 0
        for r in range(40):
            seg = slice(frp[r], frp[r + 1])
            if sort_columns:
                assert np.all(np.diff(fci[seg]) >= 0)
                same = np.diff(fci[seg]) == 0
                assert np.all(np.diff(eid[seg])[same] > 0)                   # repeated pairs in input order
            else:
                assert np.all(np.diff(eid[seg]) > 0)                         # a row keeps the input order
    assert np.array_equal(csr_from_edges_ref(er, ec, (40, 23), ev, True)[1], ci)        # column-sorted rows: the fixture itself
    ones = csr_from_edges_ref(er, ec, (40, 23))[2]
    assert ones.dtype == np.float32 and np.all(ones == 1)
    grp, gci, gva, _ = csr_from_edges_ref(np.array([0, 0, 1, 2]), np.array([0, 1, 1, 2]), (3, 3), "gcn")
    assert np.allclose(gva, [1 / 2, 1 / np.sqrt(2), 1.0, 1.0]) and gva.dtype == np.float32
    e = csr_from_edges_ref(np.zeros(0, np.int64), np.zeros(0, np.int64), (3, 4))
    assert np.array_equal(e[0], [0, 0, 0, 0]) and all(len(a) == 0 for a in e[1:])

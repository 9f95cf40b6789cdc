"""Link prediction without a GPU: the two entry points are exported and bound and refuse bad arguments before anything is
launched, the Python layer checks its arguments, and the numpy twin the GPU tests compare with (tests/linkpred_ref.py) has
the properties the contracts promise — its lookup is a dictionary's, and its negatives are uniform over the columns a row
does not store."""
import ctypes

import numpy as np
import pytest
import torch

import gcn_amd
from gcn_amd import _lib
from linkpred_ref import (find_entries_brute, find_entries_ref, lookup_fixture, lookup_queries, negative_sample_ref,
                          split_parts_ref, TRAIN)

INVALID = 1                                            # GCN_ERR_INVALID_ARG


def _host_ptr():
    buf = (ctypes.c_int32 * 64)()                      # a host array stands in for pointers only looked at, never followed
    return buf, ctypes.cast(buf, ctypes.c_void_p)


@pytest.mark.parametrize("name, nargs", [("gcn_csr_find_entries", 9), ("gcn_negative_sample_csr", 14)])
def test_new_symbols_exported_and_bound(name, nargs):
    lib = ctypes.CDLL(gcn_amd.LIB_PATH)
    assert hasattr(lib, name) and name in _lib.SIGNATURES
    fn = getattr(gcn_amd.load_library(), name)
    assert fn.restype is ctypes.c_int and fn.argtypes == _lib.SIGNATURES[name][1] and len(fn.argtypes) == nargs
    assert fn.argtypes[-1] is ctypes.c_void_p          # (void* stream last)


def test_bad_arguments_are_rejected_and_empty_problems_launch_nothing():
    lib = gcn_amd.load_library()
    _keep, p = _host_ptr()
    find, neg = lib.gcn_csr_find_entries, lib.gcn_negative_sample_csr
    good = [p, p, 3, 4, p, p, 2, p, None]
    for i in (0, 1, 4, 5, 7):                          # each pointer in turn
        args = list(good)
        args[i] = None
        assert find(*args) == INVALID, i
    for i in (2, 3, 6):                                # m, nnz, n_queries
        args = list(good)
        args[i] = -1
        assert find(*args) == INVALID, i
    assert find(None, None, 3, 4, None, None, 0, None, None) == 0                                 # no queries
    good = [p, p, 3, 3, 4, p, 2, 1, 32, 1, 0, 0, p, None]
    for i in (0, 1, 5, 12):
        args = list(good)
        args[i] = None
        assert neg(*args) == INVALID, i
    for i, bad in ((2, -1), (3, -1), (4, -1), (6, -1), (3, 0),        # m, n, nnz, n_queries; no column to draw from
                   (7, 0), (7, -1), (8, 0), (8, 65), (8, -1)):        # num_neg, max_tries
        args = list(good)
        args[i] = bad
        assert neg(*args) == INVALID, (i, bad)
    for q, k in ((2 ** 30, 2), (2, 2 ** 30), (2 ** 31 - 1, 2 ** 31 - 1)):
        args = list(good)
        args[6], args[7] = q, k
        assert neg(*args) == INVALID, (q, k)           # 2^31 slots or more: refused before anything is launched
    for tries in (1, 64):                              # the ends of the range pass the checks: no queries, nothing launched
        assert neg(None, None, 3, 3, 4, None, 0, 1, tries, 1, 0, 0, None, None) == 0
    assert neg(None, None, 3, 3, 4, None, 0, 0, 32, 1, 0, 0, None, None) == INVALID              # ... but the sizes are checked
    assert neg(None, None, 3, 3, 4, None, 0, 1, 65, 1, 0, 0, None, None) == INVALID


class _FakeAdj(gcn_amd.CsrAdjacency):
    """a CsrAdjacency shell with host arrays (the constructor refuses CPU tensors): enough to reach the checks that run
    before any native call"""

    def __init__(self, m=3, n=3, col=(0, 1, 2, 0)):
        self.m, self.n = m, n
        self.nnz = 4
        self.rowptr = torch.tensor([0, 2, 3, 4], dtype=torch.int32)
        self.col = torch.tensor(col, dtype=torch.int32)
        self.val = torch.ones(4)
        self.device = torch.device("cpu")
        self.mutable_values = False
        self.symmetric = False


BAD_IDS = (torch.tensor([0.0, 1.0]), torch.tensor([[0, 1]]), torch.tensor(1), [0, 1], torch.tensor([0, 1], dtype=torch.int16))


def test_find_edges_checks_its_arguments_in_order():
    adj, ids = _FakeAdj(), torch.tensor([0, 1], dtype=torch.int32)
    with pytest.raises(TypeError):
        gcn_amd.find_edges(torch.eye(3).to_sparse(), ids, ids)
    for bad in BAD_IDS:                                # dtype and shape come before the device
        with pytest.raises(ValueError, match="rows"):
            gcn_amd.find_edges(adj, bad, ids)
        with pytest.raises(ValueError, match="cols"):
            gcn_amd.find_edges(adj, ids, bad)
    with pytest.raises(ValueError, match="same length"):
        gcn_amd.find_edges(adj, ids, torch.tensor([0, 1, 2]))
    for fn in (lambda a: gcn_amd.find_edges(a, ids, ids), lambda a: gcn_amd.negative_sample(a, ids), gcn_amd.reverse_entries,
               lambda a: gcn_amd.split_edges(a, 0.1, 0.1), lambda a: gcn_amd.LinkNeighborLoader(a, ids, [2], 2)):
        unsorted = _FakeAdj(col=(1, 0, 2, 0))          # row 0 descends
        with pytest.raises(ValueError, match=r"csr_from_edges\(sort_columns=True\).*coalesce_csr"):
            fn(unsorted)
        assert unsorted._cols_ascend is False          # (kept on the adjacency: the second call does not look again)
        with pytest.raises(gcn_amd.GcnAmdError, match="CPU"):
            fn(_FakeAdj())
    edge = _FakeAdj(col=(0, 0, 2, 0))                  # a repeated column ascends
    with pytest.raises(gcn_amd.GcnAmdError, match="CPU"):
        gcn_amd.find_edges(edge, ids, ids.long())
    assert edge._cols_ascend is True
    with pytest.raises(ValueError, match="square"):
        gcn_amd.reverse_entries(_FakeAdj(3, 5))


def test_negative_sample_and_the_rest_check_their_arguments():
    adj, rows = _FakeAdj(), torch.tensor([0, 1], dtype=torch.int64)
    with pytest.raises(TypeError):
        gcn_amd.negative_sample(torch.eye(3).to_sparse(), rows)
    for bad in (0, -1, 1.5, None, True):
        with pytest.raises(ValueError, match="num_neg"):
            gcn_amd.negative_sample(adj, rows, num_neg=bad)
    for bad in (0, 65, 2.0, None, True):
        with pytest.raises(ValueError, match="max_tries"):
            gcn_amd.negative_sample(adj, rows, max_tries=bad)
    for bad in (-1, 2 ** 64, 1.0):
        with pytest.raises(ValueError, match="seed"):
            gcn_amd.negative_sample(adj, rows, seed=bad)
        with pytest.raises(ValueError, match="offset"):
            gcn_amd.negative_sample(adj, rows, offset=bad)
    for bad in BAD_IDS:
        with pytest.raises(ValueError, match="rows"):
            gcn_amd.negative_sample(adj, bad)
    with pytest.raises(ValueError, match="2\\^31 slots"):
        gcn_amd.negative_sample(adj, rows, num_neg=2 ** 30)
    with pytest.raises(gcn_amd.GcnAmdError, match="CPU"):
        gcn_amd.negative_sample(adj, rows)
    for bad in (torch.ones(4), torch.ones(3, dtype=torch.bool), torch.ones((4, 1), dtype=torch.bool), [True] * 4):
        with pytest.raises(ValueError, match="keep"):
            gcn_amd.edge_subgraph(adj, bad)
    with pytest.raises(gcn_amd.GcnAmdError, match="CPU"):
        gcn_amd.edge_subgraph(adj, torch.ones(4, dtype=torch.bool))
    for val, test in ((-0.1, 0.1), (0.1, 1.0), (0.5, 0.5), ("0.1", 0.1), (True, 0.1)):
        with pytest.raises(ValueError, match="frac"):
            gcn_amd.split_edges(adj, val, test)
    with pytest.raises(ValueError, match="square"):
        gcn_amd.split_edges(_FakeAdj(3, 5), 0.1, 0.1)
    with pytest.raises(ValueError, match="z_rows"):
        gcn_amd.pair_scores(torch.ones(3), torch.ones(3, 2), rows, rows)
    with pytest.raises(gcn_amd.GcnAmdError, match="CPU"):
        gcn_amd.pair_scores(torch.ones(3, 2), torch.ones(3, 2), rows, rows)
    for kw, match in ((dict(fanouts=[]), "fanouts"), (dict(fanouts=[0]), "fanout"), (dict(batch_size=0), "batch_size"),
                      (dict(num_neg=0), "num_neg"), (dict(max_tries=65), "max_tries"), (dict(seed=-1), "seed")):
        args = dict(adj=adj, eids=rows, fanouts=[2], batch_size=2)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            gcn_amd.LinkNeighborLoader(**args)


@pytest.mark.parametrize("shape", [(6000, 6000), (40, 300)])
def test_the_twin_lookup_is_a_dictionary_lookup(shape):
    m, n = shape
    rp, ci, full_row, almost_row, missing = lookup_fixture(m, n)
    lens = np.diff(rp)
    assert len(rp) == m + 1 and lens[full_row] == n and lens[almost_row] == n - 1 and (lens[almost_row + 1:] == 0).all()
    rows = np.repeat(np.arange(m), lens)
    assert ((np.diff(ci) >= 0) | (np.diff(rows) > 0)).all()                   # rows ascend ...
    assert ((np.diff(ci) == 0) & (np.diff(rows) == 0)).sum() > 10             # ... with repeated columns
    for r in np.nonzero(lens[:full_row] >= 4)[0]:                             # at the first and at the last position
        assert ci[rp[r]] == ci[rp[r] + 1] and ci[rp[r + 1] - 1] == ci[rp[r + 1] - 2]
    q_rows, q_cols = lookup_queries(rp, ci, n)
    got = find_entries_ref(rp, ci, q_rows, q_cols)
    assert np.array_equal(got, find_entries_brute(rp, ci, q_rows, q_cols))
    nnz = len(ci)
    found = got[:nnz]                                                         # the stored entries: the lowest index of each
    assert (found >= 0).all() and (found <= np.arange(nnz)).all() and (ci[found] == ci).all() and (rows[found] == rows).all()
    assert (found < np.arange(nnz)).sum() > 10 and (got[nnz:] == -1).all()    # (no other query is a stored pair)
    assert find_entries_ref(rp, ci, [almost_row, almost_row], [missing, missing + 1])[0] == -1


def test_the_twin_negatives_are_uniform_over_the_columns_a_row_does_not_store():
    """n = 64, one row with 16 stored columns, 65 536 queries of it with 16 tries each: a slot fails with probability
    (16 / 64)^16 = 2^-32, and each of the 48 other columns is drawn Binomial(65536, 1 / 48) times; 5 standard deviations"""
    n, q = 64, 65536
    stored = np.sort(np.concatenate([[0], 1 + np.random.default_rng(3).permutation(n - 1)[:15]]))   # (the row's own column too)
    rp = np.array([0, 16], np.int64)
    out = negative_sample_ref(rp, stored, n, np.zeros(q, np.int64), num_neg=1, seed=0, offset=0, max_tries=16)
    assert out.shape == (q, 1) and (out >= 0).all() and (out < n).all()
    counts = np.bincount(out[:, 0], minlength=n)
    assert (counts[stored] == 0).all()
    others = np.setdiff1d(np.arange(n), stored)
    sigma = np.sqrt(q * (1 / 48) * (47 / 48))
    worst = float(np.abs(counts[others] - q / 48).max() / sigma)
    print(f"worst bin {worst:.2f} sigma")
    assert worst <= 5.0


def test_the_twin_sampler_follows_the_contract_word_for_word():
    from util import philox4x32_10
    n, seed, offset = 1000, (5 << 32) | 7, (9 << 32) | 11
    rp, ci = np.array([0, 0, 3], np.int64), np.array([1, 500, 999], np.int64)
    for max_tries in (1, 4, 5):
        out = negative_sample_ref(rp, ci, n, [0, 1, 1, 2, -1], num_neg=3, seed=seed, offset=offset, max_tries=max_tries)
        assert (out[3:] == -1).all()                                          # rows 2 = m and -1: unusable
        T4 = 4 * ((max_tries + 3) // 4)
        for p in range(9):
            r = (0, 1, 1)[p // 3]
            want = -1
            for t in range(max_tries):
                j = p * T4 + t
                c = (int(philox4x32_10((j >> 2, 0, 11, 9), (7, 5))[j & 3]) * n) >> 32
                if c != r and not (r == 1 and c in (1, 500, 999)):
                    want = c
                    break
            assert out[p // 3, p % 3] == want
    # the self column is refused only on request, and a full row has no negative
    one = np.array([0, 4], np.int64), np.arange(4)
    assert (negative_sample_ref(*one, 4, [0] * 50, 2, max_tries=64) == -1).all()
    loop = np.array([0, 0, 0, 3], np.int64), np.array([0, 1, 3])                # row 2 of a 3 x 4 matrix lacks only column 2
    assert set(negative_sample_ref(*loop, 4, [2] * 50, 1, max_tries=64, exclude_self=False).ravel()) == {2}
    assert (negative_sample_ref(*loop, 4, [2] * 50, 1, max_tries=64, exclude_self=True) == -1).all()


def test_the_twin_split_keeps_both_directions_together():
    rng = np.random.default_rng(1)
    n = 200
    a = rng.random((n, n)) < 0.05
    a = a | a.T
    rp = np.concatenate([[0], np.cumsum(a.sum(1))])
    ci = np.nonzero(a)[1]
    rows = np.repeat(np.arange(n), np.diff(rp))
    part = split_parts_ref(rp, ci, 0.1, 0.2, seed=3, undirected=True)
    rev = find_entries_brute(rp, ci, ci, rows)
    assert (part[rev] == part).all() and (part[rows == ci] == TRAIN).all()
    frac = np.bincount(part[rows < ci], minlength=3) / (rows < ci).sum()
    assert abs(frac[1] - 0.1) < 0.03 and abs(frac[2] - 0.2) < 0.04            # (about 1900 edges: 4 standard deviations)
    free = split_parts_ref(rp, ci, 0.1, 0.2, seed=3, undirected=False)
    assert (free[rows < ci] == part[rows < ci]).all() and (free[rev] != free).any()
    assert (split_parts_ref(rp, ci, 0.0, 0.0) == TRAIN).all()

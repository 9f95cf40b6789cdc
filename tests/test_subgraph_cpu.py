"""Induced subgraphs and random walks without a GPU: the entry points are exported and bound and refuse bad arguments
before anything is launched, the Python layer and the two loaders check their arguments, and the numpy twin the GPU tests
compare with (tests/subgraph_ref.py) has the properties the contracts promise — the induced subgraph is scipy's
A[nodes][:, nodes], every step of a walk is a stored entry or a stay at a dead end, and the picks are uniform."""
import ctypes
import glob
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import gcn_amd
from gcn_amd import _lib
from subgraph_ref import induced_subgraph_ref, random_walk_ref, walk_graph, walk_keys
from util import GOLDEN, ROOT, philox4x32_10, random_rows_csr

INVALID = 1                                            # GCN_ERR_INVALID_ARG
GOLDEN_GRAPHS = sorted(glob.glob(os.path.join(GOLDEN, "reorder_*.npz")))


def _host_ptr():
    buf = (ctypes.c_int32 * 64)()                      # a host array stands in for pointers only looked at, never followed
    return buf, ctypes.cast(buf, ctypes.c_void_p)


@pytest.mark.parametrize("name, nargs", [("gcn_induced_subgraph_count_csr", 11), ("gcn_induced_subgraph_fill_csr", 13),
                                         ("gcn_random_walk_csr", 11)])
def test_new_symbols_exported_and_bound(name, nargs):
    lib = ctypes.CDLL(gcn_amd.LIB_PATH)
    assert hasattr(lib, name) and name in _lib.SIGNATURES
    fn = getattr(gcn_amd.load_library(), name)
    assert fn.restype is ctypes.c_int and fn.argtypes == _lib.SIGNATURES[name][1] and len(fn.argtypes) == nargs
    assert fn.argtypes[-1] is ctypes.c_void_p          # (void* stream last)
    text = open(os.path.join(ROOT, "include", "gcn_spmm.h")).read()
    m = re.search(r"#define\s+GCN_SUBGRAPH_WS_BYTES\s+(\d+)\b", text)
    assert m and int(m.group(1)) == _lib.SUBGRAPH_WS_BYTES


def test_bad_arguments_are_rejected_and_empty_problems_launch_nothing():
    lib = gcn_amd.load_library()
    _keep, p = _host_ptr()
    count, fill, walk = lib.gcn_induced_subgraph_count_csr, lib.gcn_induced_subgraph_fill_csr, lib.gcn_random_walk_csr
    good = [p, p, 3, 4, p, 2, p, p, p, 16, None]
    for i in (0, 1, 4, 6, 7, 8):                       # each pointer in turn
        args = list(good)
        args[i] = None
        assert count(*args) == INVALID, i
    for i, bad in ((2, -1), (3, -1), (5, -1), (9, 15)):
        args = list(good)
        args[i] = bad
        assert count(*args) == INVALID, i
    good = [p, p, 3, 4, p, 2, p, p, p, p, p, 16, None]
    for i in (0, 1, 4, 6, 7, 8, 9, 10):
        args = list(good)
        args[i] = None
        assert fill(*args) == INVALID, i
    for i, bad in ((2, -1), (3, -1), (5, -1), (11, 15)):
        args = list(good)
        args[i] = bad
        assert fill(*args) == INVALID, i
    assert count(None, None, 3, 4, None, 0, None, None, None, 0, None) == 0                       # no nodes
    assert count(None, None, 0, 0, p, 2, None, p, None, 0, None) == 0                             # no rows
    assert count(p, None, 3, 0, p, 2, None, p, None, 0, None) == 0                                # no entries
    assert fill(None, None, 3, 4, None, 0, None, None, None, None, None, 0, None) == 0
    assert fill(p, None, 3, 0, p, 2, None, p, None, None, None, 0, None) == 0
    good = [p, p, 3, 4, p, 2, 5, 0, 0, p, None]
    for i in (0, 1, 4, 9):
        args = list(good)
        args[i] = None
        assert walk(*args) == INVALID, i
    for i in (2, 3, 5, 6):                             # m, nnz, n_walks, length
        args = list(good)
        args[i] = -1
        assert walk(*args) == INVALID, i
    assert walk(None, None, 3, 4, None, 0, 5, 0, 0, None, None) == 0                              # no walks


class _FakeAdj(gcn_amd.CsrAdjacency):
    """a CsrAdjacency shell with host arrays (the constructor refuses CPU tensors): enough to reach the checks that run
    before any native call"""

    def __init__(self, m=3, n=3):
        self.m, self.n = m, n
        self.nnz = 4
        self.rowptr = torch.tensor([0, 2, 3, 4], dtype=torch.int32)
        self.col = torch.tensor([0, 1, 2, 0], dtype=torch.int32)
        self.val = torch.ones(4)
        self.device = torch.device("cpu")
        self.mutable_values = False
        self.symmetric = False


BAD_IDS = (torch.tensor([0.0, 1.0]), torch.tensor([[0, 1]]), torch.tensor(1), [0, 1], torch.tensor([0, 1], dtype=torch.int16))


def test_random_walk_checks_its_arguments_in_order():
    adj, starts = _FakeAdj(), torch.tensor([0, 1], dtype=torch.int32)
    with pytest.raises(TypeError):
        gcn_amd.random_walk(torch.eye(3).to_sparse(), starts, 2)
    with pytest.raises(ValueError, match="square"):
        gcn_amd.random_walk(_FakeAdj(3, 5), starts, 2)
    for bad in (-1, 1.5, None, True, "3"):
        with pytest.raises(ValueError, match="length"):
            gcn_amd.random_walk(adj, starts, bad)
    for bad in (-1, 2 ** 64, 1.0):
        with pytest.raises(ValueError, match="seed"):
            gcn_amd.random_walk(adj, starts, 2, seed=bad)
        with pytest.raises(ValueError, match="offset"):
            gcn_amd.random_walk(adj, starts, 2, offset=bad)
    for bad in BAD_IDS:
        with pytest.raises(ValueError, match="starts"):   # dtype and shape come before the device
            gcn_amd.random_walk(adj, bad, 2)
    for dt in (torch.int32, torch.int64):
        with pytest.raises(gcn_amd.GcnAmdError, match="CPU"):
            gcn_amd.random_walk(adj, starts.to(dt), 2)


def test_induced_subgraph_checks_its_arguments_in_order():
    adj, nodes = _FakeAdj(), torch.tensor([0, 2], dtype=torch.int64)
    with pytest.raises(TypeError):
        gcn_amd.induced_subgraph(torch.eye(3).to_sparse(), nodes)
    with pytest.raises(ValueError, match="square"):
        gcn_amd.induced_subgraph(_FakeAdj(3, 5), nodes)
    for bad in ("sym", None, 1):
        with pytest.raises(ValueError, match="values"):
            gcn_amd.induced_subgraph(adj, nodes, values=bad)
    for bad in BAD_IDS:
        with pytest.raises(ValueError, match="nodes"):
            gcn_amd.induced_subgraph(adj, bad)
    for dt in (torch.int32, torch.int64):
        with pytest.raises(gcn_amd.GcnAmdError, match="CPU"):
            gcn_amd.induced_subgraph(adj, nodes.to(dt), values="gcn")
    assert not hasattr(adj, "_sample_map")             # (refused before the vertex map is made)
    assert gcn_amd.Subgraph._fields == ("adj", "eid", "node_ids") and "node_ids" in gcn_amd.Subgraph.__doc__


def test_loaders_check_their_arguments():
    sq = _FakeAdj()
    parts = torch.tensor([1, 0, 1])
    with pytest.raises(TypeError):
        gcn_amd.ClusterLoader(torch.eye(3).to_sparse(), parts, 1)
    with pytest.raises(ValueError, match="square"):
        gcn_amd.ClusterLoader(_FakeAdj(3, 5), parts, 1)
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="clusters_per_batch"):
            gcn_amd.ClusterLoader(sq, parts, bad)
    for bad in (torch.tensor([0, 1]), torch.tensor([0.0, 1.0, 2.0]), torch.tensor([[0, 1, 2]])):
        with pytest.raises(ValueError, match="parts"):
            gcn_amd.ClusterLoader(sq, bad, 1)
    with pytest.raises(ValueError, match="values"):
        gcn_amd.ClusterLoader(sq, parts, 1, values="sym")
    with pytest.raises(ValueError, match="seed"):
        gcn_amd.ClusterLoader(sq, parts, 1, seed=-1)
    loader = gcn_amd.ClusterLoader(sq, torch.tensor([7, -2, 7]), 1)      # (cluster ids need not be consecutive)
    assert loader.num_clusters == 2 and len(loader) == 2 and len(gcn_amd.ClusterLoader(sq, parts, 2)) == 1
    assert loader._ptr == [0, 1, 3] and loader._order.tolist() == [1, 0, 2]

    idx = torch.arange(3)
    with pytest.raises(TypeError):
        gcn_amd.RandomWalkLoader(torch.eye(3).to_sparse(), idx, 2, 2, 1)
    with pytest.raises(ValueError, match="square"):
        gcn_amd.RandomWalkLoader(_FakeAdj(3, 5), idx, 2, 2, 1)
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="num_roots"):
            gcn_amd.RandomWalkLoader(sq, idx, bad, 2, 1)
        with pytest.raises(ValueError, match="batches_per_epoch"):
            gcn_amd.RandomWalkLoader(sq, idx, 2, 2, bad)
    for bad in (-1, 1.5, True):
        with pytest.raises(ValueError, match="walk_length"):
            gcn_amd.RandomWalkLoader(sq, idx, 2, bad, 1)
    for bad in (torch.tensor([0.5]), torch.zeros(0, dtype=torch.int64), torch.tensor([[0]])):
        with pytest.raises(ValueError, match="node_idx"):
            gcn_amd.RandomWalkLoader(sq, bad, 2, 2, 1)
    with pytest.raises(ValueError, match="values"):
        gcn_amd.RandomWalkLoader(sq, idx, 2, 2, 1, values="sym")
    loader = gcn_amd.RandomWalkLoader(sq, idx, 2, 2, 5)
    assert len(loader) == 5 and loader.last_offset is None and "OUT OF SCOPE" in gcn_amd.RandomWalkLoader.__doc__


# ---- the numpy twin ------------------------------------------------------------------------------------------------------------
def _sorted_rows(rp, ci):
    out = ci.copy()
    for r in range(len(rp) - 1):
        out[rp[r]:rp[r + 1]] = np.sort(ci[rp[r]:rp[r + 1]])
    return out


@pytest.mark.parametrize("path", GOLDEN_GRAPHS, ids=[os.path.basename(p)[8:-4] for p in GOLDEN_GRAPHS])
def test_twin_induced_subgraph_is_the_scipy_submatrix(path):
    g = np.load(path)
    rp, ci = g["rowptr"].astype(np.int64), g["col"].astype(np.int64)
    n = len(rp) - 1
    A = sp.csr_matrix((np.arange(1, len(ci) + 1, dtype=np.float64), ci, rp), shape=(n, n))       # value = entry index + 1
    A.sum_duplicates()
    assert A.nnz == len(ci)                            # (no pair stored twice: scipy would merge it)
    rng = np.random.default_rng(n)
    for nodes in (np.sort(rng.permutation(n)[:n // 2]), rng.permutation(n)[:n // 2], np.arange(n), np.array([n - 1]),
                  np.zeros(0, np.int64)):
        srp, sci, seid = induced_subgraph_ref(rp, ci, nodes, n)
        S = A[nodes][:, nodes].tocsr()
        S.sort_indices()
        assert np.array_equal(srp, S.indptr)
        # within a row: ascending e; sorted by column it is scipy's row, and the entry index is the value scipy carried
        for i in range(len(nodes)):
            seg = slice(srp[i], srp[i + 1])
            assert np.all(np.diff(seid[seg]) > 0)
            order = np.argsort(sci[seg], kind="stable")
            assert np.array_equal(sci[seg][order], S.indices[seg])
            assert np.array_equal(seid[seg][order] + 1, S.data[seg].astype(np.int64))
        assert np.array_equal(nodes[sci], ci[seid])


def test_twin_induced_subgraph_on_a_random_graph_with_repeated_entries():
    rp, ci = random_rows_csr(200, 200, np.random.default_rng(1).integers(0, 30, 200), seed=2)
    nodes = np.random.default_rng(3).permutation(200)[:90]
    srp, sci, seid = induced_subgraph_ref(rp, ci, nodes, 200)
    inset = np.isin(ci, nodes)
    rows = np.repeat(np.arange(200), np.diff(rp))
    assert np.array_equal(np.diff(srp), [int(inset[rows == v].sum()) for v in nodes])
    assert np.array_equal(nodes[sci], ci[seid]) and np.all(inset[seid])
    assert np.array_equal(np.sort(seid), np.flatnonzero(inset & np.isin(rows, nodes)))


def test_twin_walk_steps_are_stored_entries_or_stays():
    rp, ci = walk_graph()
    assert (np.diff(rp) == 0).sum() > 20
    starts = np.random.default_rng(5).integers(0, 300, 500)
    for length in (0, 1, 4, 5, 8):
        w = random_walk_ref(rp, ci, starts, length, seed=3, offset=9)
        assert w.shape == (500, length + 1) and np.array_equal(w[:, 0], starts)
        stays = 0
        for t in range(length):
            for v, nxt in zip(w[:, t], w[:, t + 1]):
                row = ci[rp[v]:rp[v + 1]]
                assert (len(row) == 0 and nxt == v) or nxt in row
                stays += len(row) == 0
        assert length < 4 or stays > 0
    w = random_walk_ref(rp, ci, [5, 300, -1, 7], 3)
    assert np.all(w[1:3] == -1) and np.array_equal(w[[0, 3], 0], [5, 7])
    same = random_walk_ref(rp, ci, np.full(64, 11), 8, 1, 2)            # one start, 64 walk indices: the index is in the key
    assert rp[12] - rp[11] > 1 and len({tuple(r) for r in same}) > 1


def test_twin_walk_keys_follow_the_philox_convention():
    seed, offset = (5 << 32) | 7, (9 << 32) | 11
    for length, L4 in ((1, 4), (4, 4), (5, 8), (8, 8)):
        keys = walk_keys(70, length, seed, offset)
        assert keys.shape == (70, length)
        for i in (0, 1, 69):
            for t in range(length):
                j = i * L4 + t
                words = philox4x32_10((j >> 2, 0, 11, 9), (7, 5))
                assert int(keys[i, t]) == int(words[j & 3])


@pytest.mark.parametrize("d", [2, 3, 7, 100])
@pytest.mark.parametrize("length", [1, 5])
@pytest.mark.parametrize("seed, offset", [(0, 0), (1, 7)])
def test_twin_picks_are_uniform(d, length, seed, offset):
    """every row of the graph is the columns 0 .. d - 1, so the vertex after a step IS the pick: 65 536 walks, and per step
    and per pick a count that is Binomial(65536, 1 / d); the bound is 5 of its standard deviations"""
    n_walks = 65536
    rp = np.arange(d + 1, dtype=np.int64) * d
    ci = np.tile(np.arange(d), d)
    w = random_walk_ref(rp, ci, np.zeros(n_walks, np.int64), length, seed, offset)
    sigma = np.sqrt(n_walks * (1 / d) * (1 - 1 / d))
    worst = 0.0
    for t in range(1, length + 1):
        counts = np.bincount(w[:, t], minlength=d)
        assert counts.sum() == n_walks and len(counts) == d
        worst = max(worst, float(np.abs(counts - n_walks / d).max() / sigma))
    print(f"d {d}, length {length}, (seed, offset) ({seed}, {offset}): worst bin {worst:.2f} sigma")
    assert worst <= 5.0

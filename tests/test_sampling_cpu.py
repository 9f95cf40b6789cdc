"""Neighbour sampling without a GPU: the entry point is exported and bound, bad arguments are refused and empty problems
accepted before anything is launched, the Python layer checks its arguments in the documented order, and the numpy
reference the GPU tests compare with (tests/sampling_ref.py) has the properties the contract promises — uniformity, the
tie rule on a pair of equal keys that exists, the relabelling on a hand-written graph."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import gcn_amd
from gcn_amd import _lib
from sampling_ref import (TIE_SEARCH, entry_keys, relabel_ref, sample_blocks_ref, sample_neighbors_ref, sample_row, tie_row,
                          tied_pairs)
from util import ROOT, philox4x32_10

NEW = ["gcn_sample_neighbors_csr"]
INVALID = 1                                            # GCN_ERR_INVALID_ARG


@pytest.mark.parametrize("name", NEW)
def test_new_symbols_exported_and_bound(name):
    lib = ctypes.CDLL(gcn_amd.LIB_PATH)
    assert hasattr(lib, name)
    assert name in _lib.SIGNATURES
    fn = getattr(gcn_amd.load_library(), name)
    assert fn.restype is ctypes.c_int
    assert fn.argtypes == _lib.SIGNATURES[name][1]
    assert len(fn.argtypes) == 15
    assert fn.argtypes[-1] is ctypes.c_void_p          # (void* stream last)
    assert fn.argtypes[-2] is ctypes.c_size_t          # (the workspace's size before it)
    assert fn.argtypes[7] is ctypes.c_uint64 and fn.argtypes[8] is ctypes.c_uint64      # seed, offset


def test_header_constants_match_the_binding():
    text = open(os.path.join(ROOT, "include", "gcn_spmm.h")).read()
    m = re.search(r"#define\s+GCN_SAMPLE_LONG_ROW\s+(\d+)\b", text)
    assert m and int(m.group(1)) == _lib.SAMPLE_LONG_ROW
    m = re.search(r"#define\s+GCN_SAMPLE_WS_BYTES\s+(\d+)\b", text)
    assert m and int(m.group(1)) == _lib.SAMPLE_WS_BYTES


def test_bad_arguments_are_rejected():
    fn = gcn_amd.load_library().gcn_sample_neighbors_csr
    buf = (ctypes.c_int32 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)              # a host array stands in for pointers only looked at, never followed
    good = [p, p, 3, 4, p, 2, 5, 0, 0, p, p, p, p, 16, None]
    for i in (0, 1, 4, 9, 10, 11, 12):                 # each pointer in turn
        args = list(good)
        args[i] = None
        assert fn(*args) == INVALID, i
    for i, bad in ((2, -1), (3, -1), (5, -1), (6, 0), (13, 15)):      # m, nnz, n_seeds, fanout 0, a short workspace
        args = list(good)
        args[i] = bad
        assert fn(*args) == INVALID, i
    assert fn(None, None, 0, 0, None, 0, 0, 0, 0, None, None, None, None, 0, None) == INVALID   # fanout 0 on an empty problem too


def test_problems_without_output_are_ok_and_launch_nothing():
    fn = gcn_amd.load_library().gcn_sample_neighbors_csr
    buf = (ctypes.c_int32 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert fn(None, None, 3, 4, None, 0, 5, 0, 0, None, None, None, None, 0, None) == 0          # no seeds
    assert fn(None, None, 0, 0, p, 2, -1, 0, 0, p, None, None, None, 0, None) == 0               # no rows
    assert fn(p, None, 3, 0, p, 2, 5, 1, 2, p, None, None, None, 0, None) == 0                   # no entries


class _FakeAdj(gcn_amd.CsrAdjacency):
    """a CsrAdjacency shell with host arrays (the constructor refuses CPU tensors): enough to reach the checks that run
    before any native call"""

    def __init__(self, m=3, n=5):
        self.m, self.n = m, n
        self.nnz = 4
        self.rowptr = torch.tensor([0, 2, 3, 4], dtype=torch.int32)
        self.col = torch.tensor([0, 1, 4, 0], dtype=torch.int32)
        self.val = torch.ones(4)
        self.device = torch.device("cpu")
        self.mutable_values = False


def test_sample_neighbors_checks_its_arguments_in_order():
    adj = _FakeAdj()
    seeds = torch.tensor([0, 1], dtype=torch.int32)
    with pytest.raises(TypeError):
        gcn_amd.sample_neighbors(torch.eye(3).to_sparse(), seeds, 2)
    for bad in (0, -2, 1.5, None, True, "3"):
        with pytest.raises(ValueError, match="fanout"):
            gcn_amd.sample_neighbors(adj, seeds, bad)
    for bad in (-1, 2 ** 64, 1.0):
        with pytest.raises(ValueError, match="seed"):
            gcn_amd.sample_neighbors(adj, seeds, 2, seed=bad)
        with pytest.raises(ValueError, match="offset"):
            gcn_amd.sample_neighbors(adj, seeds, 2, offset=bad)
    for bad in (torch.tensor([0.0, 1.0]), torch.tensor([[0, 1]]), torch.tensor(1), [0, 1], torch.tensor([0, 1], dtype=torch.int16)):
        with pytest.raises(ValueError, match="seeds"):   # dtype and shape come before the device
            gcn_amd.sample_neighbors(adj, bad, 2)
    for dt in (torch.int32, torch.int64):
        with pytest.raises(gcn_amd.GcnAmdError, match="CPU"):
            gcn_amd.sample_neighbors(adj, seeds.to(dt), 2)


def test_sample_blocks_and_loader_check_their_arguments():
    seeds = torch.tensor([0, 1], dtype=torch.int64)
    with pytest.raises(TypeError):
        gcn_amd.sample_blocks(torch.eye(3).to_sparse(), seeds, [2])
    with pytest.raises(ValueError, match="square"):
        gcn_amd.sample_blocks(_FakeAdj(3, 5), seeds, [2])
    sq = _FakeAdj(3, 3)
    with pytest.raises(ValueError, match="fanouts"):
        gcn_amd.sample_blocks(sq, seeds, [])
    with pytest.raises(ValueError, match="fanout"):
        gcn_amd.sample_blocks(sq, seeds, [2, 0])
    with pytest.raises(gcn_amd.GcnAmdError, match="CPU"):
        gcn_amd.sample_blocks(sq, seeds, [2, 2])
    assert not hasattr(sq, "_sample_map")              # (refused before the vertex map is made)
    with pytest.raises(TypeError):
        gcn_amd.NeighborLoader(torch.eye(3).to_sparse(), seeds, [2], 1)
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="batch_size"):
            gcn_amd.NeighborLoader(sq, seeds, [2], bad)
    with pytest.raises(ValueError, match="fanout"):
        gcn_amd.NeighborLoader(sq, seeds, [0], 1)
    with pytest.raises(ValueError, match="node_idx"):
        gcn_amd.NeighborLoader(sq, torch.tensor([0.5]), [2], 1)
    assert len(gcn_amd.NeighborLoader(sq, torch.arange(3), [2, 2], 2)) == 2
    assert len(gcn_amd.NeighborLoader(sq, torch.arange(3), [2], 3)) == 1


def test_graphsage_constructs_and_bipartite_sageconv_checks_shapes():
    model = gcn_amd.GraphSAGE(12, 8, 3, num_layers=3, aggr="max", dropout=0.25)
    assert [(l.in_features, l.out_features, l.aggr) for l in model.layers] == [(12, 8, "max"), (8, 8, "max"), (8, 3, "max")]
    assert repr(model) == "GraphSAGE (12 -> 8 -> 3, layers=3, aggr=max, dropout=0.25)"
    assert len(gcn_amd.GraphSAGE(4, 9, 2, num_layers=1).layers) == 1
    assert gcn_amd.GraphSAGE(4, 4, 2, root_weight=False).layers[0].weight_root is None
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="num_layers"):
            gcn_amd.GraphSAGE(4, 4, 2, num_layers=bad)
    with pytest.raises(ValueError, match="dropout"):
        gcn_amd.GraphSAGE(4, 4, 2, dropout=1.0)
    with pytest.raises(ValueError, match="aggr"):
        gcn_amd.GraphSAGE(4, 4, 2, aggr="median")
    adj = _FakeAdj(3, 5)
    with pytest.raises(ValueError, match="blocks"):
        model(torch.ones(5, 12), [])
    layer = gcn_amd.SAGEConv(2, 2)
    for bad in ((torch.ones(4, 2), torch.ones(3, 2)), (torch.ones(5, 2), torch.ones(5, 2)), (torch.ones(5, 2),),
                (torch.ones(5), torch.ones(3, 2))):
        with pytest.raises(ValueError):
            layer(bad, adj)
    with pytest.raises(ValueError, match="square"):    # the single-tensor form keeps its rule and its error
        layer(torch.ones(5, 2), adj)
    with pytest.raises(gcn_amd.GcnAmdError, match="CPU"):      # a well-shaped pair passes the checks and reaches the aggregator
        layer((torch.ones(5, 2), torch.ones(3, 2)), adj)


# ---- the numpy reference ------------------------------------------------------------------------------------------------------
def test_reference_keys_follow_the_dropout_convention():
    e = np.array([0, 1, 2, 3, 4, 7, 4 * 12345 + 2, (1 << 22) - 1])
    seed, offset = (5 << 32) | 7, (9 << 32) | 11
    keys = entry_keys(e, seed, offset)
    for x, k in zip(e, keys):
        words = philox4x32_10((x >> 2, 0, 11, 9), (7, 5))
        assert int(k) == int(words[x & 3])


def test_reference_selects_the_smallest_keys_in_entry_order():
    b, e, f = 13, 13 + 40, 10
    sel = sample_row(b, e, f, 3, 4)
    keys = entry_keys(np.arange(b, e), 3, 4)
    assert len(sel) == f and np.all(np.diff(sel) > 0) and sel.min() >= b and sel.max() < e
    assert keys[sel - b].max() <= np.delete(keys, sel - b).min()
    assert np.array_equal(sample_row(b, e, 40, 3, 4), np.arange(b, e))               # d <= f: the whole row
    assert np.array_equal(sample_row(b, e, -1, 3, 4), np.arange(b, e))
    assert len(sample_row(5, 5, 3, 0, 0)) == 0
    rp, c, eid = sample_neighbors_ref([0, 2, 2, 9], np.arange(9) * 2, [2, 1, 0, 2], 3, 1, 2)
    assert rp.tolist() == [0, 3, 3, 5, 8] and eid[3:5].tolist() == [0, 1]
    assert np.array_equal(eid[:3], eid[5:]) and np.array_equal(c, 2 * eid)          # the same vertex: the same neighbours


def test_reference_is_uniform():
    """one row of 40 entries, f = 10, seed 7, offsets 0 .. 1999: every entry is drawn 500 times in expectation and 5 sigma
    of Binomial(2000, 1/4) is 97"""
    counts = np.zeros(40, np.int64)
    for offset in range(2000):
        counts[sample_row(0, 40, 10, 7, offset)] += 1
    assert counts.sum() == 20000
    assert counts.min() >= 500 - 97 and counts.max() <= 500 + 97, (counts.min(), counts.max())


def test_reference_ties_exist_and_the_lower_entry_wins():
    pairs = tied_pairs(1, 0, TIE_SEARCH)
    assert len(pairs) == 2106                          # (N^2 / 2^33 predicts 2048)
    e1, e2, key = pairs[0]
    assert (e1, e2, key) == (2568115, 2569214, 3442188123)
    gaps = np.array([p[1] - p[0] for p in pairs])
    assert (gaps < 4096).sum() == 5 and (gaps > 8192).sum() == 2099
    b, e, f = tie_row(e1, e2, key)
    assert e - b == 1106
    sel = sample_row(b, e, f, 1, 0)
    assert len(sel) == f and e1 in sel and e2 not in sel
    keys = entry_keys(sel, 1, 0)
    assert int(keys.max()) == key and int((keys == key).sum()) == 1


def test_reference_relabelling_on_a_hand_written_graph():
    # 6 vertices; row v lists its neighbours
    nbrs = {0: [1, 2], 1: [0, 3, 5], 2: [2], 3: [], 4: [0, 5], 5: [4, 1, 1]}
    rowptr = np.cumsum([0] + [len(nbrs[v]) for v in range(6)])
    col = np.concatenate([np.array(nbrs[v], np.int64) for v in range(6)])
    val = np.arange(len(col), dtype=np.float32) + 1
    src, local = relabel_ref([4, 1], [0, 5, 0, 3, 5])
    assert src.tolist() == [4, 1, 0, 3, 5] and local.tolist() == [2, 4, 2, 3, 4]
    blocks, input_ids = sample_blocks_ref(rowptr, col, val, [4, 1], [-1, -1])
    inner, outer = blocks[1], blocks[0]                # blocks[-1] has the seeds as its rows
    assert inner["num_dst"] == 2 and inner["src_ids"].tolist() == [4, 1, 0, 3, 5]
    assert inner["rowptr"].tolist() == [0, 2, 5] and inner["eid"].tolist() == [6, 7, 2, 3, 4]
    assert inner["col"].tolist() == [2, 4, 2, 3, 4] and inner["val"].tolist() == [7, 8, 3, 4, 5]
    # the next hop's rows are the inner src; new vertices: 2 (from 0) — 1, 4 and 5 are already there
    assert outer["num_dst"] == 5 and outer["src_ids"].tolist() == [4, 1, 0, 3, 5, 2] == input_ids.tolist()
    assert outer["rowptr"].tolist() == [0, 2, 5, 7, 7, 10]
    assert outer["eid"].tolist() == [6, 7, 2, 3, 4, 0, 1, 8, 9, 10]
    assert outer["col"].tolist() == [2, 4, 2, 3, 4, 1, 5, 0, 1, 1]
    assert np.array_equal(outer["src_ids"][:5], inner["src_ids"])

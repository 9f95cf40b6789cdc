"""Max / min / sum / mean aggregation without a GPU: the two entry points are exported and bound with the argument types
gcn_amd/_lib.py declares, bad arguments are refused and empty problems accepted before anything is launched, the workspace
macro of the header and the Python sizing agree, gcn_amd.aggregate checks its arguments in the documented order (no CPU
path), and SAGEConv constructs with the documented parameters, repr and errors."""
import ctypes
import importlib
import math
import os
import re

import pytest
import torch

import gcn_amd
from gcn_amd import _lib
from util import ROOT

aggregate_mod = importlib.import_module("gcn_amd.aggregate")    # (gcn_amd.aggregate itself is the function)
NEW = ["gcn_aggregate_csr", "gcn_aggregate_backward_csr"]
INVALID = 1                                            # GCN_ERR_INVALID_ARG
F32, BF16, MAX, MIN = 0, 1, 0, 1


@pytest.mark.parametrize("name", NEW)
def test_new_symbols_exported_and_bound(name):
    lib = ctypes.CDLL(gcn_amd.LIB_PATH)
    assert hasattr(lib, name)
    assert name in _lib.SIGNATURES
    fn = getattr(gcn_amd.load_library(), name)
    assert fn.restype is ctypes.c_int
    assert fn.argtypes == _lib.SIGNATURES[name][1]
    assert len(fn.argtypes) == 14
    assert fn.argtypes[-1] is ctypes.c_void_p          # (void* stream last)
    assert fn.argtypes[-2] is ctypes.c_size_t          # (the workspace's size before it)


def test_header_constants_match_the_binding():
    text = open(os.path.join(ROOT, "include", "gcn_spmm.h")).read()
    assert re.search(r"#define\s+GCN_REDUCE_MAX\s+0\b", text) and re.search(r"#define\s+GCN_REDUCE_MIN\s+1\b", text)
    assert (_lib.REDUCE_MAX, _lib.REDUCE_MIN) == (0, 1)
    m = re.search(r"#define\s+GCN_AGGREGATE_WS_BYTES\(nnz, k\)\s+\(16 \+ 16 \* \(size_t\)\(k\) \* \(\(\(size_t\)\(nnz\) \+ (\d+)\) / (\d+)\)\)", text)
    assert m and int(m.group(1)) + 1 == int(m.group(2)) == aggregate_mod._CHUNK
    for nnz, k in ((0, 1), (1, 1), (4096, 128), (4097, 128), (114_848_857, 200)):
        assert aggregate_mod._ws_bytes(nnz, k) == 16 + 16 * k * ((nnz + 4095) // 4096)


def test_bad_arguments_are_rejected():
    lib = gcn_amd.load_library()
    big = 1 << 30
    buf = (ctypes.c_int32 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)              # a host array stands in for pointers only looked at, never followed
    fwd, bwd = lib.gcn_aggregate_csr, lib.gcn_aggregate_backward_csr
    assert fwd(None, None, 3, 3, 4, None, F32, 8, MAX, None, None, None, big, None) == INVALID
    assert bwd(None, None, None, 3, 3, 4, None, F32, None, 8, None, None, big, None) == INVALID
    for i in (0, 1, 5, 9, 10, 11):                     # each pointer of the forward in turn
        args = [p, p, 3, 3, 4, p, F32, 8, MAX, p, p, p, big, None]
        args[i] = None
        assert fwd(*args) == INVALID, i
    for i in (0, 1, 2, 6, 8, 10, 11):
        args = [p, p, p, 3, 3, 4, p, F32, p, 8, p, p, big, None]
        args[i] = None
        assert bwd(*args) == INVALID, i
    assert fwd(p, p, 3, 3, 4, p, F32, 0, MAX, p, p, p, big, None) == INVALID        # k < 1
    assert fwd(p, p, 3, 3, 4, p, F32, 8, 2, p, p, p, big, None) == INVALID          # unknown op
    assert fwd(p, p, 3, 3, 4, p, 2, 8, MIN, p, p, p, big, None) == INVALID          # unknown dtype
    assert fwd(p, p, -1, 3, 4, p, F32, 8, MAX, p, p, p, big, None) == INVALID
    assert fwd(p, p, 3, 3, -4, p, BF16, 8, MAX, p, p, p, big, None) == INVALID
    assert bwd(p, p, p, 3, 3, 4, p, 7, p, 8, p, p, big, None) == INVALID
    assert bwd(p, p, p, 3, 3, 4, p, BF16, p, 0, p, p, big, None) == INVALID
    short = aggregate_mod._ws_bytes(4, 8) - 1                                         # a workspace one byte short
    assert fwd(p, p, 3, 3, 4, p, F32, 8, MAX, p, p, p, short, None) == INVALID
    assert bwd(p, p, p, 3, 3, 4, p, F32, p, 8, p, p, short, None) == INVALID
    # an unknown op or k < 1 is refused on an empty problem too
    assert fwd(None, None, 0, 0, 0, None, F32, 8, 5, None, None, None, 0, None) == INVALID
    assert fwd(None, None, 0, 0, 0, None, F32, 0, MAX, None, None, None, 0, None) == INVALID


def test_problems_without_output_rows_are_ok_and_launch_nothing():
    lib = gcn_amd.load_library()
    assert lib.gcn_aggregate_csr(None, None, 0, 0, 0, None, F32, 8, MAX, None, None, None, 0, None) == 0
    assert lib.gcn_aggregate_csr(None, None, 0, 7, 0, None, BF16, 3, MIN, None, None, None, 0, None) == 0
    assert lib.gcn_aggregate_backward_csr(None, None, None, 0, 5, 0, None, F32, None, 8, None, None, 0, None) == 0


class _FakeAdj(gcn_amd.CsrAdjacency):
    """a CsrAdjacency shell with host arrays (the constructor refuses CPU tensors): enough to reach the checks that run
    before any native call"""

    def __init__(self):
        self.m, self.n = 3, 5
        self.nnz = 4
        self.rowptr = torch.tensor([0, 2, 3, 4], dtype=torch.int32)
        self.col = torch.tensor([0, 1, 4, 0], dtype=torch.int32)
        self.val = torch.ones(4)
        self.device = torch.device("cpu")
        self.mutable_values = False
        self._plan = None
        self._transpose = None


def test_aggregate_checks_its_arguments_in_order():
    assert gcn_amd.aggregate is aggregate_mod.aggregate
    adj = _FakeAdj()
    with pytest.raises(TypeError):
        gcn_amd.aggregate(torch.eye(3).to_sparse(), torch.ones(3, 2))
    with pytest.raises(ValueError, match="reduce"):
        gcn_amd.aggregate(adj, torch.ones(5, 2), "median")
    for bad in (torch.ones(3, 2), torch.ones(5), torch.ones(5, 2, 1), torch.ones(5, 0), [[1.0]] * 5):
        with pytest.raises(ValueError):                # the shape comes before the device: a ValueError, CPU tensor or not
            gcn_amd.aggregate(adj, bad, "max")
    for reduce in ("max", "min", "sum", "mean"):
        with pytest.raises(gcn_amd.GcnAmdError, match="CPU"):
            gcn_amd.aggregate(adj, torch.ones(5, 2, requires_grad=True), reduce)
    with pytest.raises(gcn_amd.GcnAmdError):           # (the device comes before the dtype)
        gcn_amd.aggregate(adj, torch.ones(5, 2, dtype=torch.float64), "max")


@pytest.mark.parametrize("aggr", ["mean", "max", "min", "sum"])
def test_sage_conv_constructs(aggr):
    layer = gcn_amd.SAGEConv(12, 8, aggr=aggr)
    sd = layer.state_dict()
    assert set(sd) == {"weight_neigh", "weight_root", "bias"}
    assert sd["weight_neigh"].shape == (12, 8) == sd["weight_root"].shape and sd["bias"].shape == (8,)
    bound = 1.0 / math.sqrt(8)                          # (as the GCN layers: uniform in +-1/sqrt(out_features))
    for v in sd.values():
        assert float(v.abs().max()) <= bound and float(v.abs().max()) > 0
    assert repr(layer) == f"SAGEConv (12 -> 8, aggr={aggr})"
    other = gcn_amd.SAGEConv(12, 8, aggr=aggr)
    other.load_state_dict(sd)
    for k, v in other.state_dict().items():
        assert torch.equal(v, sd[k])
    bare = gcn_amd.SAGEConv(12, 8, aggr=aggr, root_weight=False, with_bias=False)
    assert set(bare.state_dict()) == {"weight_neigh"}
    assert bare.weight_root is None and bare.bias is None
    assert repr(bare) == f"SAGEConv (12 -> 8, aggr={aggr}, no root weight)"


def test_sage_conv_default_and_unknown_aggr():
    assert gcn_amd.SAGEConv(4, 4).aggr == "mean"
    for bad in ("median", "", None, "MAX"):
        with pytest.raises(ValueError, match="aggr"):
            gcn_amd.SAGEConv(4, 4, aggr=bad)

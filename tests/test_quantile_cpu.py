"""Quantile aggregation without a GPU: gcn_aggregate_quantile_csr_f32 refuses bad arguments before any device pointer is
read, gcn_amd.aggregate_quantile checks its arguments in the documented order (no CPU path), and MedianConv constructs with
the documented parameters, repr and errors."""
import ctypes
import math

import pytest
import torch

import gcn_amd
from test_aggregate_cpu import _FakeAdj

P = ctypes.c_void_p(64)                                # a non-null "device pointer" that must never be read
GOOD = dict(rowptr=P, col=P, m=4, n=4, nnz=8, x=P, k=4, q=(0.5,), out=P, arg=P, ws=P, ws_bytes=16)


def forward(**kw):
    a = {**GOOD, **kw}
    q = (ctypes.c_double * max(len(a["q"]), 1))(*a["q"]) if a["q"] is not None else None
    return gcn_amd.load_library().gcn_aggregate_quantile_csr_f32(a["rowptr"], a["col"], a["m"], a["n"], a["nnz"], a["x"], a["k"], q,
                                                                 a.get("nq", len(a["q"]) if a["q"] is not None else 1), a["out"],
                                                                 a["arg"], a["ws"], a["ws_bytes"], None)


@pytest.mark.parametrize("bad", [dict(q=(), nq=0), dict(q=(0.1, 0.2, 0.3, 0.4, 0.5)), dict(q=None), dict(q=(-0.01,)), dict(q=(0.5, 1.01)),
                                 dict(q=(float("nan"),)), dict(q=(float("inf"),)), dict(k=0), dict(m=-1), dict(nnz=-1), dict(rowptr=None),
                                 dict(col=None), dict(x=None), dict(out=None), dict(arg=None), dict(ws=None), dict(ws_bytes=15)])
def test_entry_point_argument_errors(bad):
    assert forward(**bad) == 1                          # GCN_ERR_INVALID_ARG
    assert forward(**{"m": 0, **bad}) == (0 if set(bad) <= {"rowptr", "col", "x", "out", "arg", "ws", "ws_bytes"} else 1)   # no rows: only the sizes and q count


def test_aggregate_quantile_checks_its_arguments_in_order():
    adj = _FakeAdj()
    with pytest.raises(TypeError):
        gcn_amd.aggregate_quantile(torch.eye(3).to_sparse(), torch.ones(3, 2))
    for bad in (-0.1, 1.5, float("nan"), (), (0.1, 0.2, 0.3, 0.4, 0.5), (0.5, 2.0), "median", None):
        with pytest.raises(ValueError, match="q must be"):                         # q comes before the shape
            gcn_amd.aggregate_quantile(adj, torch.ones(3, 2), bad)
    for bad in (torch.ones(3, 2), torch.ones(5), torch.ones(5, 0), [[1.0]] * 5):
        with pytest.raises(ValueError, match="x must be"):                         # the shape comes before the device
            gcn_amd.aggregate_quantile(adj, bad)
    with pytest.raises(gcn_amd.GcnAmdError, match="CPU"):
        gcn_amd.aggregate_quantile(adj, torch.ones(5, 2, requires_grad=True), (0.25, 0.75))
    with pytest.raises(gcn_amd.GcnAmdError, match="CPU"):                          # (the device comes before the dtype)
        gcn_amd.aggregate_quantile(adj, torch.ones(5, 2, dtype=torch.float64))


def test_median_conv_constructs():
    layer = gcn_amd.MedianConv(12, 8, root_weight=True)
    sd = layer.state_dict()
    assert set(sd) == {"weight", "weight_root", "bias"}
    assert sd["weight"].shape == (12, 8) == sd["weight_root"].shape and sd["bias"].shape == (8,)
    for v in sd.values():                                  # (as the GCN layers: uniform in +-1/sqrt(out_features))
        assert 0 < float(v.abs().max()) <= 1.0 / math.sqrt(8)
    assert repr(layer) == "MedianConv (12 -> 8, q=0.5)"
    bare = gcn_amd.MedianConv(12, 8, q=0.25, with_bias=False)
    assert set(bare.state_dict()) == {"weight"} and bare.weight_root is None and bare.bias is None
    assert repr(bare) == "MedianConv (12 -> 8, q=0.25, no root weight)"
    for bad in (-0.1, 1.1, float("nan"), (0.25, 0.75), "median", None):
        with pytest.raises(ValueError, match="q must be"):
            gcn_amd.MedianConv(4, 4, q=bad)

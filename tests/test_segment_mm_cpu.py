"""The grouped matrix product without a GPU: the three symbols are declared and bound, and the argument errors of
segment_matmul, RowGather, TypedLinear and RGCNConv(grouped=True) come before any device work."""
import os

import pytest
import torch

import gcn_amd
from gcn_amd import _lib, build
from util import ROOT

NAMES = {"gcn_segment_mm_ws_bytes": 5, "gcn_segment_mm_f32": 15, "gcn_segment_mm_wgrad_f32": 16}


@pytest.mark.parametrize("name", list(NAMES))
def test_the_symbols_are_declared_bound_and_exported(name):
    header = open(os.path.join(ROOT, "include", "gcn_spmm.h")).read()
    assert f"int {name}(" in header and len(_lib.SIGNATURES[name][1]) == NAMES[name]
    assert hasattr(gcn_amd.load_library(), name)
    assert "segment_mm.hip" in build.SOURCES and "segment_mm.h" in build.HEADERS
    assert f"#define GCN_SEGMENT_MM_CHUNK {_lib.SEGMENT_MM_CHUNK}\n" in header


def test_segment_matmul_argument_errors():
    x, ptr, w = torch.ones(4, 3), torch.tensor([0, 2, 4], dtype=torch.int32), torch.ones(2, 3, 5)
    idx = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(TypeError):
        gcn_amd.segment_matmul(x, ptr, w, index=[0, 1, 2, 3])
    for bad in (dict(x=torch.ones(4)), dict(segptr=ptr.long()), dict(segptr=ptr[:2]), dict(weight=torch.ones(2, 4, 5)),
                dict(weight=torch.ones(2, 3)), dict(index=idx.long()), dict(scale=torch.ones(3)),
                dict(scale=torch.ones(4, requires_grad=True))):
        with pytest.raises(ValueError):
            gcn_amd.segment_matmul(**{**dict(x=x, segptr=ptr, weight=w), **bad})
    for bad in (dict(), dict(x=x.double()), dict(weight=w.half()), dict(scale=torch.ones(4))):          # CPU tensors, dtypes
        with pytest.raises(gcn_amd.GcnAmdError):
            gcn_amd.segment_matmul(**{**dict(x=x, segptr=ptr, weight=w), **bad})
    with pytest.raises(gcn_amd.GcnAmdError):
        gcn_amd.RowGather(idx, 4)
    with pytest.raises(ValueError):
        gcn_amd.RowGather(idx.long(), 4)


def test_layer_argument_errors():
    for args in ((0, 4, 2), (4, 4, True), (4, 2.0, 2)):
        with pytest.raises(ValueError):
            gcn_amd.TypedLinear(*args)
    lin = gcn_amd.TypedLinear(3, 5, 2)
    assert tuple(lin.weight.shape) == (2, 3, 5) and tuple(lin.bias.shape) == (2, 5) and gcn_amd.TypedLinear(3, 5, 2, bias=False).bias is None
    for x, ptr in ((torch.ones(4, 3), [0, 4]), (torch.ones(4, 2), [0, 2, 4])):
        with pytest.raises(ValueError):
            lin(x, torch.tensor(ptr, dtype=torch.int32))
    with pytest.raises(gcn_amd.GcnAmdError):
        lin(torch.ones(4, 3), torch.tensor([0, 2, 4], dtype=torch.int32))
    with pytest.raises(ValueError, match="num_bases"):
        gcn_amd.RGCNConv(4, 4, 3, num_bases=2, grouped=True)
    grouped, typed = gcn_amd.RGCNConv(4, 6, 3, grouped=True), gcn_amd.RGCNConv(4, 6, 3)
    assert grouped.grouped and not typed.grouped and {k: tuple(v.shape) for k, v in grouped.state_dict().items()} == {k: tuple(v.shape) for k, v in typed.state_dict().items()}
    with pytest.raises(TypeError):
        gcn_amd.relation_transform_aggregate(None, torch.ones(2, 2), torch.ones(1, 2, 2))

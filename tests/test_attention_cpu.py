"""Attention aggregation without a GPU: the five edge-softmax entry points are exported and bound, null pointers and bad
sizes are refused, CPU tensors raise (no CPU path), wrong shapes are ValueErrors, the fused form insists on a mutable
adjacency, and GraphAttention constructs and round-trips its state on the CPU."""
import ctypes

import pytest
import torch

import gcn_amd
from gcn_amd import _lib

NEW = ["gcn_edge_softmax_csr_f32", "gcn_edge_softmax_backward_csr_f32", "gcn_gat_edge_softmax_csr_f32",
       "gcn_gat_edge_softmax_backward_csr_f32", "gcn_segment_sum_csr_f32"]
INVALID = 1                                            # GCN_ERR_INVALID_ARG


@pytest.mark.parametrize("name", NEW)
def test_new_symbols_exported_and_bound(name):
    lib = ctypes.CDLL(gcn_amd.LIB_PATH)
    assert hasattr(lib, name)
    assert name in _lib.SIGNATURES
    fn = getattr(gcn_amd.load_library(), name)
    assert fn.restype is ctypes.c_int
    assert fn.argtypes == _lib.SIGNATURES[name][1]
    assert fn.argtypes[-1] is ctypes.c_void_p          # (void* stream last)


def test_null_pointers_and_bad_sizes_are_rejected():
    lib = gcn_amd.load_library()
    big = 1 << 20
    assert lib.gcn_edge_softmax_csr_f32(None, 3, 4, None, None, None, big, None) == INVALID
    assert lib.gcn_edge_softmax_backward_csr_f32(None, 3, 4, None, None, None, None, big, None) == INVALID
    assert lib.gcn_gat_edge_softmax_csr_f32(None, None, 3, 4, None, None, 0.2, None, None, big, None) == INVALID
    assert lib.gcn_gat_edge_softmax_backward_csr_f32(None, None, 3, 4, None, None, 0.2, None, None, None, None, None, big,
                                                     None) == INVALID
    assert lib.gcn_segment_sum_csr_f32(None, 3, 4, None, None, None, None, big, None) == INVALID
    # negative sizes, whatever the pointers
    assert lib.gcn_edge_softmax_csr_f32(None, -1, 4, None, None, None, big, None) == INVALID
    assert lib.gcn_segment_sum_csr_f32(None, 3, -4, None, None, None, None, big, None) == INVALID
    # a host array stands in for the pointers the check looks at before anything is launched: a workspace too small
    buf = (ctypes.c_int32 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.gcn_edge_softmax_csr_f32(p, 3, 4, p, p, p, 8, None) == INVALID
    assert lib.gcn_edge_softmax_csr_f32(p, 3, 4, None, p, p, big, None) == INVALID
    assert lib.gcn_gat_edge_softmax_backward_csr_f32(p, p, 3, 4, p, p, 0.2, p, p, p, None, p, big, None) == INVALID


def test_empty_problems_are_ok_and_launch_nothing():
    lib = gcn_amd.load_library()
    assert lib.gcn_edge_softmax_csr_f32(None, 0, 0, None, None, None, 0, None) == 0
    assert lib.gcn_edge_softmax_backward_csr_f32(None, 5, 0, None, None, None, None, 0, None) == 0
    assert lib.gcn_gat_edge_softmax_csr_f32(None, None, 0, 7, None, None, 0.2, None, None, 0, None) == 0
    assert lib.gcn_gat_edge_softmax_backward_csr_f32(None, None, 0, 0, None, None, 0.2, None, None, None, None, None, 0, None) == 0
    assert lib.gcn_segment_sum_csr_f32(None, 4, 0, None, None, None, None, 0, None) == 0


class _FakeAdj(gcn_amd.CsrAdjacency):
    """a CsrAdjacency shell with host arrays (the constructor refuses CPU tensors): enough to reach the checks that run
    before any native call"""

    def __init__(self, mutable=True):
        self.m = self.n = 3
        self.nnz = 4
        self.rowptr = torch.tensor([0, 2, 3, 4], dtype=torch.int32)
        self.col = torch.tensor([0, 1, 2, 0], dtype=torch.int32)
        self.val = torch.ones(4)
        self.device = torch.device("cpu")
        self.mutable_values = mutable
        self._plan = None
        self._transpose = None


def test_cpu_tensors_raise():
    adj = _FakeAdj()
    with pytest.raises(gcn_amd.GcnAmdError):
        gcn_amd.edge_softmax(adj, torch.ones(4, requires_grad=True))
    with pytest.raises(gcn_amd.GcnAmdError):
        gcn_amd.gat_edge_softmax(adj, torch.ones(3), torch.ones(3))
    with pytest.raises(gcn_amd.GcnAmdError):
        gcn_amd.segment_sum(adj.rowptr, torch.ones(4))


def test_wrong_length_or_rank_is_a_value_error():
    adj = _FakeAdj()
    for bad in (torch.ones(5), torch.ones(3), torch.ones(2, 2)):
        with pytest.raises(ValueError):
            gcn_amd.edge_softmax(adj, bad)
    for bad in (torch.ones(4), torch.ones(3, 1)):
        with pytest.raises(ValueError):
            gcn_amd.gat_edge_softmax(adj, bad, torch.ones(3))
        with pytest.raises(ValueError):
            gcn_amd.gat_edge_softmax(adj, torch.ones(3), bad)


def test_gat_edge_softmax_needs_a_mutable_adjacency():
    adj = _FakeAdj(mutable=False)
    with pytest.raises(gcn_amd.GcnAmdError, match="mutable_values"):
        gcn_amd.gat_edge_softmax(adj, torch.ones(3), torch.ones(3))


@pytest.mark.parametrize("heads,concat", [(1, True), (4, True), (4, False)])
def test_graph_attention_constructs_and_round_trips(heads, concat):
    layer = gcn_amd.GraphAttention(12, 8, heads=heads, concat=concat, negative_slope=0.1)
    sd = layer.state_dict()
    assert set(sd) == {"weight", "att_dst", "att_src", "bias"}
    assert sd["weight"].shape == (12, heads * 8) and sd["att_dst"].shape == (heads, 8) == sd["att_src"].shape
    assert sd["bias"].shape == ((heads * 8,) if concat else (8,))
    other = gcn_amd.GraphAttention(12, 8, heads=heads, concat=concat)
    other.load_state_dict(sd)
    for k, v in other.state_dict().items():
        assert torch.equal(v, sd[k])
    nobias = gcn_amd.GraphAttention(12, 8, heads=heads, concat=concat, with_bias=False)
    assert set(nobias.state_dict()) == {"weight", "att_dst", "att_src"}

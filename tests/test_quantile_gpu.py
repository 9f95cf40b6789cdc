"""Quantile / median aggregation on the GPU (gcn_amd/csrc/aggregate_quantile.hip, gcn_amd.aggregate_quantile, MedianConv).

A selection rounds nothing, so out is compared BY BITS and arg for equality against tests/quantile_ref.py.  One matrix
serves every case: row lengths 0 .. 3, b - 1, b, b + 1 around every class bound of the unit (the sorting networks of 4, 8,
16 and 32 inputs; the wave's radix select up to 2048 entries; the workgroup's beyond) and one row of 70 000 entries (past
a 16-bit count), columns drawn with repeats from 97 nodes, features from six levels so that ties are the rule."""
import functools

import numpy as np
import pytest
import torch

import gcn_amd
from quantile_ref import quantile_ref
from test_aggregate_gpu import bits, graph, make_adj
from util import offset_view

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N = 97
LENS = [0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 0, 31, 32, 33, 2047, 2048, 2049, 70000, 1]
RP = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int32)
COL = np.random.default_rng(0).integers(0, N, int(RP[-1])).astype(np.int32)
ALLQ = (0.0, 0.25, 0.5, 0.75, 1.0)


@functools.lru_cache(None)
def adjacency():
    return gcn_amd.CsrAdjacency(torch.from_numpy(RP).to(DEV), torch.from_numpy(COL).to(DEV), torch.ones(len(COL), device=DEV),
                                (len(LENS), N))


@functools.lru_cache(None)
def case(k):
    """(x, the reference's out and arg for the five quantiles of ALLQ), computed once per width"""
    x = np.random.default_rng(k).choice(np.array([-2, -1, -0.0, 0.0, 1, 2], np.float32), (N, k))
    x[5, 0], x[50, 0] = np.inf, -np.inf
    x[[11, 60], k - 1] = np.nan
    return x, quantile_ref(RP, COL, x, ALLQ)


def expected(k, qs):
    _x, (out, arg) = case(k)
    at = np.concatenate([np.arange(k) + ALLQ.index(q) * k for q in qs])
    return out[:, at], arg[:, at]


@pytest.mark.parametrize("q", [0.0, 0.25, 0.5, 1.0, (0.25, 0.5, 0.75)])
@pytest.mark.parametrize("k", [1, 3, 4, 64, 65, 130])
def test_out_and_arg_match_the_reference_by_bits(k, q):
    qs = q if isinstance(q, tuple) else (q,)
    out, arg = gcn_amd.aggregate_quantile(adjacency(), torch.from_numpy(case(k)[0]).to(DEV), q, return_arg=True)
    want_out, want_arg = expected(k, qs)
    assert out.shape == arg.shape == (len(LENS), len(qs) * k) and out.dtype == torch.float32 and arg.dtype == torch.int32
    assert torch.equal(arg.cpu(), torch.from_numpy(want_arg))
    assert np.array_equal(bits(out), bits(want_out))


def test_operand_one_element_off_a_16_byte_boundary():
    x, _flat = offset_view(case(4)[0], 1, torch.float32, DEV)
    out, arg = gcn_amd.aggregate_quantile(adjacency(), x, (0.25, 0.5, 0.75), return_arg=True)
    want_out, want_arg = expected(4, (0.25, 0.5, 0.75))
    assert torch.equal(arg.cpu(), torch.from_numpy(want_arg)) and np.array_equal(bits(out), bits(want_out))


@pytest.mark.parametrize("q", [0.5, (0.25, 0.5, 0.75)])
@pytest.mark.parametrize("k", [4, 65])
def test_gradient_goes_to_the_selected_entries(k, q):
    qs = q if isinstance(q, tuple) else (q,)
    x = torch.from_numpy(case(k)[0]).to(DEV).requires_grad_(True)
    g = torch.from_numpy(np.random.default_rng(1).integers(-3, 4, (len(LENS), len(qs) * k)).astype(np.float32))
    out, arg = gcn_amd.aggregate_quantile(adjacency(), x, q, return_arg=True)
    out.backward(g.to(DEV))
    arg = arg.cpu().long()
    assert torch.equal(arg, torch.from_numpy(expected(k, qs)[1]).long())
    want = torch.zeros(N, k, dtype=torch.float64)          # integer-valued g: every sum is exact in fp32 and fp64
    rows = arg >= 0
    cols = torch.arange(k).repeat(len(qs)).expand(len(LENS), -1)
    want.index_put_((torch.from_numpy(COL).long()[arg[rows]], cols[rows]), g.double()[rows], accumulate=True)
    assert np.array_equal(bits(x.grad), bits(want.float()))


def test_two_calls_and_a_captured_replay_give_the_same_bits():
    adj, q = adjacency(), (0.25, 0.5, 0.75)
    x = torch.from_numpy(case(4)[0]).to(DEV).requires_grad_(True)
    gout = torch.ones(len(LENS), 12, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                          # one eager call: the workspaces and the transpose exist
        first = gcn_amd.aggregate_quantile(adj, x, q)
        first.backward(gout)
    torch.cuda.current_stream().wait_stream(side)
    assert np.array_equal(bits(first), bits(gcn_amd.aggregate_quantile(adj, x, q)))
    x.grad = None
    graph_ = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph_):
        out = gcn_amd.aggregate_quantile(adj, x, q)
        out.backward(gout)
    for seed in (2, 3):
        with torch.no_grad():
            x.copy_(torch.from_numpy(np.random.default_rng(seed).integers(-2, 3, (N, 4)).astype(np.float32)))
        graph_.replay()
        torch.cuda.synchronize()
        xe = x.detach().clone().requires_grad_(True)
        oe = gcn_amd.aggregate_quantile(adj, xe, q)
        oe.backward(gout)
        assert np.array_equal(bits(out), bits(oe)) and np.array_equal(bits(x.grad), bits(xe.grad))


@pytest.mark.parametrize("sampled", [False, True])
def test_median_conv_is_the_written_out_composition(sampled):
    _rp, _col, n = graph("cora")
    adj = make_adj("cora")
    torch.manual_seed(3)
    layer = gcn_amd.MedianConv(16, 8, root_weight=True).to(DEV)
    x = torch.randn(n, 16)
    if sampled:
        (blk,), ids = gcn_amd.sample_blocks(adj, torch.arange(0, n, 5, device=DEV), [4], seed=1)
        adj, x = blk.adj, x[ids.cpu().long()]
    xd = x.to(DEV).requires_grad_(True)
    out = layer((xd, xd[:adj.m]) if sampled else xd, adj)
    with torch.no_grad():
        want = gcn_amd.aggregate_quantile(adj, xd @ layer.weight, 0.5) + xd[:adj.m] @ layer.weight_root + layer.bias
    assert out.shape == (adj.m, 8) and np.array_equal(bits(out), bits(want))
    out.backward(torch.randn(adj.m, 8, device=DEV))
    for t in (layer.weight.grad, layer.weight_root.grad, layer.bias.grad, xd.grad):
        assert bool(torch.isfinite(t).all()) and float(t.abs().max()) > 0

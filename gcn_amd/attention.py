"""Attention over edges: the softmax over the stored entries of each row of a CSR pattern ("edge softmax"), its form
fused with GAT scores, and CSR row sums of a per-entry array — the autograd surface of gcn_amd/csrc/edge_softmax.hip.

    p = gcn_amd.edge_softmax(adj, scores)                    # scores: nnz fp32 values in adj's CSR order
    p = gcn_amd.gat_edge_softmax(adj, a_dst, a_src, 0.2)     # scores leaky_relu(a_dst[row] + a_src[col]), never stored
    out = gcn_amd.spmm(adj, h, values=p)                     # the weighted aggregation

The kernels take no plan and only enqueue, so all of this runs inside a captured step.  Unlike ``torch.softmax`` a row
whose scores are all -inf gets zeros, not NaN (a fully masked row stays usable).  There is no CPU path: CPU tensors raise.
"""
import torch

from . import _lib
from .spmm import CsrAdjacency, _ptr, _stream_ptr

_CHUNK = 8192                # entries per workspace partial: GCN_EDGE_WS_BYTES in include/gcn_spmm.h


def _ws_bytes(nnz):
    return 16 + 16 * ((int(nnz) + _CHUNK - 1) // _CHUNK)


def _workspace(owner, nnz, device):
    """the scratch the kernels want (a flag and the partials of rows longer than 8192 entries), kept on the adjacency:
    allocated at the first call — so before a capture, with the plans — and shared by its calls, which one stream orders"""
    ws = getattr(owner, "_edge_ws", None)
    if ws is None or ws.numel() < _ws_bytes(nnz) or ws.device != device:
        ws = torch.empty(_ws_bytes(nnz), dtype=torch.uint8, device=device)
        owner._edge_ws = ws
    return ws


def _entry_tensor(adj, t, what):
    """the checks of spmm(values=...): shape first (ValueError), then device and dtype (GcnAmdError)"""
    if not isinstance(t, torch.Tensor) or t.dim() != 1 or t.numel() != adj.nnz:
        raise ValueError(f"{what} must be a 1-D tensor of nnz = {adj.nnz} entries in CSR order")
    if not t.is_cuda:
        raise _lib.GcnAmdError(f"{what} must be a CUDA/HIP tensor (no CPU path in gcn_amd)")
    if t.dtype != torch.float32:
        raise _lib.GcnAmdError(f"{what} must be fp32")


def _node_tensors(pairs):
    """shapes of all of them first (ValueError), then device and dtype (GcnAmdError)"""
    for t, count, what in pairs:
        if not isinstance(t, torch.Tensor) or t.dim() != 1 or t.numel() != count:
            raise ValueError(f"{what} must be a 1-D tensor of {count} entries")
    for t, _count, what in pairs:
        if not t.is_cuda:
            raise _lib.GcnAmdError(f"{what} must be a CUDA/HIP tensor (no CPU path in gcn_amd)")
        if t.dtype != torch.float32:
            raise _lib.GcnAmdError(f"{what} must be fp32")


def _segment_sum_raw(owner, rowptr, m, x, perm, out):
    nnz = int(x.numel())
    if m == 0 or nnz == 0:
        return out.zero_()
    ws = _workspace(owner, nnz, x.device)
    with torch.cuda.device(x.device):
        st = _lib.load().gcn_segment_sum_csr_f32(_ptr(rowptr), m, nnz, _ptr(x), _ptr(perm) if perm is not None else None,
                                                 _ptr(out), _ptr(ws), ws.numel(), _stream_ptr(x.device))
    _lib.check(st, "gcn_segment_sum_csr_f32")
    return out


class _SegmentSumHolder:
    """keeps the workspace of segment_sum calls that have no adjacency to keep it on"""


_loose = {}                  # (device index, stream handle) -> holder: calls on different streams never share a workspace


def _loose_holder(device):
    key = (device.index if device.index is not None else torch.cuda.current_device(),
           torch.cuda.current_stream(device).cuda_stream)
    holder = _loose.get(key)
    if holder is None:
        holder = _loose[key] = _SegmentSumHolder()
    return holder


def segment_sum(rowptr, x, perm=None):
    """out[r] = sum of x[e] over rowptr[r] <= e < rowptr[r+1] (x[perm[e]] with an int32 permutation `perm`): plain CSR row
    sums of a per-entry fp32 device array, in a fixed order (no atomics) — gcn_segment_sum_csr_f32.  No autograd.
    Its scratch is kept per (device, stream), so calls on different streams do not share one."""
    if not (isinstance(rowptr, torch.Tensor) and rowptr.dim() == 1 and rowptr.numel() >= 1):
        raise ValueError("segment_sum: rowptr must be a 1-D tensor of m + 1 entries")
    if not isinstance(x, torch.Tensor) or x.dim() != 1:
        raise ValueError("segment_sum: x must be a 1-D tensor with one entry per stored entry")
    if perm is not None and (not isinstance(perm, torch.Tensor) or perm.shape != x.shape):
        raise ValueError("segment_sum: perm must have one entry per entry of x")
    if not (rowptr.is_cuda and x.is_cuda and (perm is None or perm.is_cuda)):
        raise _lib.GcnAmdError("segment_sum needs CUDA/HIP tensors (no CPU path in gcn_amd)")
    if x.dtype != torch.float32 or rowptr.dtype != torch.int32 or (perm is not None and perm.dtype != torch.int32):
        raise _lib.GcnAmdError("segment_sum: x must be fp32, rowptr and perm int32")
    m = int(rowptr.numel()) - 1
    out = torch.empty(m, dtype=torch.float32, device=x.device)
    return _segment_sum_raw(_loose_holder(x.device), rowptr.contiguous(), m, x.detach().contiguous(),
                            perm.contiguous() if perm is not None else None, out)


class _EdgeSoftmaxFunction(torch.autograd.Function):
    """p = softmax of `scores` over each row's stored entries; saves p: ds = p (g - sum_row p g)"""

    @staticmethod
    def forward(ctx, adj, scores):
        s = scores.detach().contiguous()
        p = torch.empty_like(s)
        if adj.m and adj.nnz:
            ws = _workspace(adj, adj.nnz, s.device)
            with torch.cuda.device(s.device):
                st = _lib.load().gcn_edge_softmax_csr_f32(_ptr(adj.rowptr), adj.m, adj.nnz, _ptr(s), _ptr(p), _ptr(ws),
                                                          ws.numel(), _stream_ptr(s.device))
            _lib.check(st, "gcn_edge_softmax_csr_f32")
        ctx.adj = adj
        ctx.save_for_backward(p)
        return p

    @staticmethod
    def backward(ctx, g):
        (p,) = ctx.saved_tensors
        adj = ctx.adj
        g = g.contiguous()
        ds = torch.empty_like(p)
        if adj.m and adj.nnz:
            ws = _workspace(adj, adj.nnz, p.device)
            with torch.cuda.device(p.device):
                st = _lib.load().gcn_edge_softmax_backward_csr_f32(_ptr(adj.rowptr), adj.m, adj.nnz, _ptr(p), _ptr(g), _ptr(ds),
                                                                   _ptr(ws), ws.numel(), _stream_ptr(p.device))
            _lib.check(st, "gcn_edge_softmax_backward_csr_f32")
        return None, ds


def edge_softmax(adj, scores):
    """p[e] = exp(scores[e] - max_row) / sum_row exp(scores[e'] - max_row) over the stored entries of each row of `adj`
    (any CsrAdjacency: only its rowptr is used, its values are ignored).  `scores`: 1-D fp32 device tensor of nnz entries
    in adj's CSR order; differentiable.  Empty rows have no entries; an all -inf row gets zeros (torch.softmax: NaN); a NaN
    stays in its row.  ValueError for a wrong shape, GcnAmdError for a CPU tensor or a dtype other than fp32."""
    if not isinstance(adj, CsrAdjacency):
        raise TypeError("edge_softmax: adj must be a CsrAdjacency")
    _entry_tensor(adj, scores, "edge_softmax: scores")
    return _EdgeSoftmaxFunction.apply(adj, scores)


class _GatEdgeSoftmaxFunction(torch.autograd.Function):
    """p = edge softmax of leaky_relu(a_dst[row] + a_src[col]); backward recomputes the scores from a_dst, a_src:
    grad_a_dst = row sums of ds (same kernel), grad_a_src = column sums of ds = row sums over the transpose's rowptr of
    ds read through the transpose permutation (segment sum: one writer per output, no atomics)."""

    @staticmethod
    def forward(ctx, adj, a_dst, a_src, slope):
        ad, asrc = a_dst.detach().contiguous(), a_src.detach().contiguous()
        p = torch.empty(adj.nnz, dtype=torch.float32, device=ad.device)
        if adj.m and adj.nnz:
            ws = _workspace(adj, adj.nnz, ad.device)
            with torch.cuda.device(ad.device):
                st = _lib.load().gcn_gat_edge_softmax_csr_f32(_ptr(adj.rowptr), _ptr(adj.col), adj.m, adj.nnz, _ptr(ad),
                                                              _ptr(asrc), slope, _ptr(p), _ptr(ws), ws.numel(),
                                                              _stream_ptr(ad.device))
            _lib.check(st, "gcn_gat_edge_softmax_csr_f32")
        ctx.adj, ctx.slope = adj, slope
        ctx.save_for_backward(ad, asrc, p)
        return p

    @staticmethod
    def backward(ctx, g):
        ad, asrc, p = ctx.saved_tensors
        adj = ctx.adj
        dev = p.device
        g = g.contiguous()
        ds = torch.empty_like(p)
        g_dst = torch.empty(adj.m, dtype=torch.float32, device=dev)
        g_src = torch.empty(adj.n, dtype=torch.float32, device=dev)
        if not (adj.m and adj.nnz):
            return None, g_dst.zero_(), g_src.zero_(), None
        ws = _workspace(adj, adj.nnz, dev)
        with torch.cuda.device(dev):
            st = _lib.load().gcn_gat_edge_softmax_backward_csr_f32(_ptr(adj.rowptr), _ptr(adj.col), adj.m, adj.nnz, _ptr(ad),
                                                                   _ptr(asrc), ctx.slope, _ptr(p), _ptr(g), _ptr(ds),
                                                                   _ptr(g_dst), _ptr(ws), ws.numel(), _stream_ptr(dev))
        _lib.check(st, "gcn_gat_edge_softmax_backward_csr_f32")
        if ctx.needs_input_grad[2]:
            t = adj._mutable_transpose()                 # (its pattern and permutation; its values are not touched)
            perm = getattr(adj, "_tperm32", None)
            if perm is None:
                perm = adj._tperm32 = adj._tperm.to(torch.int32)
            _segment_sum_raw(adj, t.rowptr, adj.n, ds, perm, g_src)
        else:
            g_src = None
        return None, g_dst, g_src, None


def gat_edge_softmax(adj, a_dst, a_src, negative_slope=0.2):
    """The edge softmax of the GAT scores s[e] = leaky_relu(a_dst[row(e)] + a_src[col(e)], negative_slope), computed inside
    the kernel: the nnz-sized score array is never written.  a_dst: [m] fp32, a_src: [n] fp32, both differentiable.
    `adj` must have been made with mutable_values=True — only because grad_a_src sums ds by column through the transpose
    permutation such an adjacency keeps (and the result is meant for spmm(adj, h, values=p), which needs it anyway)."""
    if not isinstance(adj, CsrAdjacency):
        raise TypeError("gat_edge_softmax: adj must be a CsrAdjacency")
    if not adj.mutable_values:
        raise _lib.GcnAmdError("gat_edge_softmax needs an adjacency made with mutable_values=True (grad_a_src is summed "
                               "through the transpose permutation only a mutable adjacency keeps)")
    _node_tensors([(a_dst, adj.m, "gat_edge_softmax: a_dst"), (a_src, adj.n, "gat_edge_softmax: a_src")])
    return _GatEdgeSoftmaxFunction.apply(adj, a_dst, a_src, float(negative_slope))

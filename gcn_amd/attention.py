"""Attention over edges: the softmax over the stored entries of each row of a CSR pattern ("edge softmax"), its form
fused with GAT scores, and CSR row sums of a per-entry array — the autograd surface of gcn_amd/csrc/edge_softmax.hip.

    p = gcn_amd.edge_softmax(adj, scores)                    # scores: nnz fp32 values in adj's CSR order
    p = gcn_amd.gat_edge_softmax(adj, a_dst, a_src, 0.2)     # scores leaky_relu(a_dst[row] + a_src[col]), never stored
    out = gcn_amd.spmm(adj, h, values=p)                     # the weighted aggregation

All heads of a multi-head layer go through one pass: the same functions take 2-D operands with an entry's or a node's H
heads contiguous (the 1-D forms are their H = 1 case, through the same kernels' one-head instantiation), and the
aggregation and its score counterpart (gcn_amd/csrc/multihead.hip) are

    p = gcn_amd.edge_softmax(adj, scores)                    # scores [nnz, H] -> p [nnz, H]
    p = gcn_amd.gat_edge_softmax(adj, a_dst, a_src, 0.2)     # a_dst [m, H], a_src [n, H] -> p [nnz, H]
    out = gcn_amd.spmm_heads(adj, x, p)                      # x [n, H*F]: out[r, hF+j] = sum_e p[e, h] x[col[e], hF+j]
    s = gcn_amd.sddmm_heads(adj, a, b, heads)                # s[e, h] = <a[row(e), head h], b[col[e], head h]>
    s = gcn_amd.gatv2_scores(adj, h_dst, h_src, att, 0.2)    # s[e, h] = <att[h], leaky_relu(h_dst[row(e)] + h_src[col[e]])>

The kernels take no plan and only enqueue, so all of this runs inside a captured step.  Unlike ``torch.softmax`` a row
whose scores are all -inf gets zeros, not NaN (a fully masked row stays usable).  There is no CPU path: CPU tensors raise.
"""
import ctypes
import functools

import torch

from . import _lib
from ._lib import call
from .spmm import CsrAdjacency, Scratch


@functools.lru_cache(maxsize=None)
def _ws_need(query, nnz, heads, k):
    """bytes of scratch the library's `query` (gcn_heads_ws_bytes, gcn_gatv2_ws_bytes) asks for: a flag and the chunk
    partials of long rows"""
    need = ctypes.c_size_t(0)
    call(query, 0, nnz, heads, k, ctypes.byref(need))
    return need.value


def _workspace(owner, nnz, device, heads=1, k=1):
    """the scratch the kernels want (gcn_heads_ws_bytes: a flag and the chunk partials of long rows): the "edge" buffer of
    the owner's Scratch — an adjacency's, or the Scratch itself for a segment_sum without one — shared by the owner's
    softmax, segment-sum and heads calls, which one stream orders.  Only the size rule lives here; the keeping is Scratch's"""
    keeper = owner._scratch if isinstance(owner, CsrAdjacency) else owner
    return keeper.get("edge", _ws_need("gcn_heads_ws_bytes", int(nnz), int(heads), int(k)), device)


def _check_adj(adj, what):
    if not isinstance(adj, CsrAdjacency):
        raise TypeError(f"{what}: adj must be a CsrAdjacency")


def _fp32_tensors(items):
    """items: (tensor, shape, what, form).  The checks of spmm(values=...): the shapes of all of them first (ValueError
    "`what` must be `form`"; None in a shape: any size, and the width of a 2-D tensor is at least 1), then device and dtype
    (GcnAmdError)"""
    for t, shape, what, form in items:
        if (not isinstance(t, torch.Tensor) or t.dim() != len(shape) or (t.dim() == 2 and t.shape[1] < 1)
                or any(want is not None and have != want for have, want in zip(t.shape, shape))):
            raise ValueError(f"{what} must be {form}")
    for t, _shape, what, _form in items:
        if not t.is_cuda:
            raise _lib.GcnAmdError(f"{what} must be a CUDA/HIP tensor (no CPU path in gcn_amd)")
        if t.dtype != torch.float32:
            raise _lib.GcnAmdError(f"{what} must be fp32")


def _heads_of(t):
    """H of a per-entry or per-node array: [count, H], or [count] for one head"""
    return int(t.shape[1]) if t.dim() == 2 else 1


def _segment_sum_raw(owner, rowptr, rows, x, perm, out):
    """out [rows] or [rows, H] = the row sums over rowptr of x [nnz] or [nnz, H] (read through perm)"""
    nnz, heads = int(x.shape[0]), _heads_of(x)
    if rows == 0 or nnz == 0:
        return out.zero_()
    ws = _workspace(owner, nnz, x.device, heads, heads)
    call("gcn_segment_sum_heads_csr_f32", rowptr, rows, nnz, heads, x, perm, out, ws, ws.numel(), device=x.device)
    return out


_loose = {}                  # (device index, stream handle) -> Scratch of the segment_sum calls that have no adjacency to keep
                             # it on: calls on different streams never share a workspace


def _loose_scratch(device):
    key = (device.index if device.index is not None else torch.cuda.current_device(),
           torch.cuda.current_stream(device).cuda_stream)
    scratch = _loose.get(key)
    if scratch is None:
        scratch = _loose[key] = Scratch()
    return scratch


def segment_sum(rowptr, x, perm=None):
    """out[r] = sum of x[e] over rowptr[r] <= e < rowptr[r+1] (x[perm[e]] with an int32 permutation `perm`): plain CSR row
    sums of a per-entry fp32 device array, in a fixed order (no atomics) — gcn_segment_sum_heads_csr_f32.  No autograd.
    x may be 2-D [nnz, H] (an entry's heads contiguous): the result is [m, H], from one pass over the entries.
    Its scratch is kept per (device, stream), so calls on different streams do not share one."""
    if not (isinstance(rowptr, torch.Tensor) and rowptr.dim() == 1 and rowptr.numel() >= 1):
        raise ValueError("segment_sum: rowptr must be a 1-D tensor of m + 1 entries")
    if not isinstance(x, torch.Tensor) or x.dim() not in (1, 2) or (x.dim() == 2 and x.shape[1] < 1):
        raise ValueError("segment_sum: x must be a 1-D tensor with one entry per stored entry, or 2-D [nnz, H]")
    if perm is not None and (not isinstance(perm, torch.Tensor) or perm.shape != x.shape[:1]):
        raise ValueError("segment_sum: perm must have one entry per entry of x")
    if not (rowptr.is_cuda and x.is_cuda and (perm is None or perm.is_cuda)):
        raise _lib.GcnAmdError("segment_sum needs CUDA/HIP tensors (no CPU path in gcn_amd)")
    if x.dtype != torch.float32 or rowptr.dtype != torch.int32 or (perm is not None and perm.dtype != torch.int32):
        raise _lib.GcnAmdError("segment_sum: x must be fp32, rowptr and perm int32")
    m = int(rowptr.numel()) - 1
    out = torch.empty((m,) + tuple(x.shape[1:]), dtype=torch.float32, device=x.device)
    return _segment_sum_raw(_loose_scratch(x.device), rowptr.contiguous(), m, x.detach().contiguous(),
                            perm.contiguous() if perm is not None else None, out)


class _EdgeSoftmaxFunction(torch.autograd.Function):
    """p = per-head softmax of `scores` ([nnz] or [nnz, H]) over each row's stored entries; saves p: ds = p (g - sum_row p g)"""

    @staticmethod
    def forward(ctx, adj, scores):
        s = scores.detach().contiguous()
        p = torch.empty_like(s)
        heads = _heads_of(s)
        if adj.m and adj.nnz:
            ws = _workspace(adj, adj.nnz, s.device, heads, heads)
            call("gcn_edge_softmax_heads_csr_f32", adj.rowptr, adj.m, adj.nnz, heads, s, p, ws, ws.numel(), device=s.device)
        ctx.adj = adj
        ctx.save_for_backward(p)
        return p

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        (p,) = ctx.saved_tensors
        adj = ctx.adj
        g = g.contiguous()
        ds = torch.empty_like(p)
        heads = _heads_of(p)
        if adj.m and adj.nnz:
            ws = _workspace(adj, adj.nnz, p.device, heads, heads)
            call("gcn_edge_softmax_heads_backward_csr_f32", adj.rowptr, adj.m, adj.nnz, heads, p, g, ds, ws, ws.numel(),
                 device=p.device)
        return None, ds


def edge_softmax(adj, scores):
    """p[e] = exp(scores[e] - max_row) / sum_row exp(scores[e'] - max_row) over the stored entries of each row of `adj`
    (any CsrAdjacency: only its rowptr is used, its values are ignored).  `scores`: 1-D fp32 device tensor of nnz entries
    in adj's CSR order; differentiable.  Empty rows have no entries; an all -inf row gets zeros (torch.softmax: NaN); a NaN
    stays in its row.  `scores` may be 2-D [nnz, H]: the softmax is taken per head, all heads in one pass (p is [nnz, H]).
    ValueError for a wrong shape, GcnAmdError for a CPU tensor or a dtype other than fp32."""
    _check_adj(adj, "edge_softmax")
    if isinstance(scores, torch.Tensor) and scores.dim() == 2:           # [nnz, H]: all heads in one pass
        _fp32_tensors([(scores, (adj.nnz, None), "edge_softmax: scores", f"a 2-D tensor [nnz = {adj.nnz}, H] in CSR order")])
    else:
        _fp32_tensors([(scores, (adj.nnz,), "edge_softmax: scores", f"a 1-D tensor of nnz = {adj.nnz} entries in CSR order")])
    return _EdgeSoftmaxFunction.apply(adj, scores)


class _GatEdgeSoftmaxFunction(torch.autograd.Function):
    """p = per-head edge softmax of leaky_relu(a_dst[row] + a_src[col]) (a_dst [m] or [m, H]); the backward recomputes the
    scores from a_dst, a_src: grad_a_dst = row sums of ds (same kernel), grad_a_src = column sums of ds = row sums over the
    transposed pattern's rowptr of ds read through its permutation (segment sum: one writer per output, no atomics; one
    gather brings an entry's H values)."""

    @staticmethod
    def forward(ctx, adj, a_dst, a_src, slope):
        ad, asrc = a_dst.detach().contiguous(), a_src.detach().contiguous()
        heads = _heads_of(ad)
        p = torch.empty((adj.nnz,) + tuple(ad.shape[1:]), dtype=torch.float32, device=ad.device)
        if adj.m and adj.nnz:
            ws = _workspace(adj, adj.nnz, ad.device, heads, heads)
            call("gcn_gat_edge_softmax_heads_csr_f32", adj.rowptr, adj.col, adj.m, adj.nnz, heads, ad, asrc, slope, p, ws,
                 ws.numel(), device=ad.device)
        ctx.adj, ctx.slope = adj, slope
        ctx.save_for_backward(ad, asrc, p)
        return p

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        ad, asrc, p = ctx.saved_tensors
        adj = ctx.adj
        dev = p.device
        heads = _heads_of(p)
        g = g.contiguous()
        ds = torch.empty_like(p)
        g_dst = torch.empty_like(ad)
        g_src = torch.empty_like(asrc)
        if not (adj.m and adj.nnz):
            return None, g_dst.zero_(), g_src.zero_(), None
        ws = _workspace(adj, adj.nnz, dev, heads, heads)
        call("gcn_gat_edge_softmax_heads_backward_csr_f32", adj.rowptr, adj.col, adj.m, adj.nnz, heads, ad, asrc, ctx.slope, p,
             g, ds, g_dst, ws, ws.numel(), device=dev)
        if ctx.needs_input_grad[2]:
            trp, _trow, tperm = adj.tpattern()
            _segment_sum_raw(adj, trp, adj.n, ds, tperm, g_src)
        else:
            g_src = None
        return None, g_dst, g_src, None


def gat_edge_softmax(adj, a_dst, a_src, negative_slope=0.2):
    """The edge softmax of the GAT scores s[e] = leaky_relu(a_dst[row(e)] + a_src[col(e)], negative_slope), computed inside
    the kernel: the nnz-sized score array is never written.  a_dst: [m] fp32, a_src: [n] fp32, both differentiable.
    `adj` must have been made with mutable_values=True — only because grad_a_src sums ds by column through the transpose
    permutation such an adjacency keeps (and the result is meant for spmm(adj, h, values=p), which needs it anyway).
    With a_dst [m, H] and a_src [n, H] all heads run in one pass, p is [nnz, H] (for spmm_heads) and any adjacency will do."""
    _check_adj(adj, "gat_edge_softmax")
    if isinstance(a_dst, torch.Tensor) and isinstance(a_src, torch.Tensor) and (a_dst.dim() == 2 or a_src.dim() == 2):
        heads = int(a_dst.shape[-1])                     # a_dst [m, H], a_src [n, H]: all heads in one pass, any adjacency
        _fp32_tensors([(a_dst, (adj.m, heads), "gat_edge_softmax: a_dst", f"a 2-D tensor [{adj.m}, {heads}]"),
                       (a_src, (adj.n, heads), "gat_edge_softmax: a_src", f"a 2-D tensor [{adj.n}, {heads}]")])
    else:
        if not adj.mutable_values:
            raise _lib.GcnAmdError("gat_edge_softmax needs an adjacency made with mutable_values=True (grad_a_src is summed "
                                   "through the transpose permutation only a mutable adjacency keeps)")
        _fp32_tensors([(a_dst, (adj.m,), "gat_edge_softmax: a_dst", f"a 1-D tensor of {adj.m} entries"),
                       (a_src, (adj.n,), "gat_edge_softmax: a_src", f"a 1-D tensor of {adj.n} entries")])
    return _GatEdgeSoftmaxFunction.apply(adj, a_dst, a_src, float(negative_slope))


# ---- the gathers of all heads in one pass (gcn_amd/csrc/multihead.hip) ------------------------------------------------------------
def _spmm_heads_raw(adj, rowptr, idx, perm, rows, vals, x, heads):
    """out [rows, k] of gcn_spmm_heads_csr_f32 over (rowptr, idx, perm); vals [nnz, H], x [*, k]"""
    k = int(x.shape[1])
    out = torch.empty(rows, k, dtype=torch.float32, device=x.device)
    if rows == 0 or adj.nnz == 0:
        return out.zero_()
    ws = _workspace(adj, adj.nnz, x.device, heads, k)
    call("gcn_spmm_heads_csr_f32", rowptr, idx, perm, rows, adj.nnz, heads, k, vals, x, out, ws, ws.numel(), device=x.device)
    return out


def _sddmm_heads_raw(adj, a, b, heads):
    k = int(a.shape[1])
    out = torch.empty(adj.nnz, heads, dtype=torch.float32, device=a.device)
    if adj.m == 0 or adj.nnz == 0:
        return out
    ws = _workspace(adj, adj.nnz, a.device, heads, k)
    call("gcn_sddmm_heads_csr_f32", adj.rowptr, adj.col, adj.m, adj.nnz, heads, k, a, b, out, ws, ws.numel(), device=a.device)
    return out


class _SpmmHeadsFunction(torch.autograd.Function):
    """out = spmm_heads(adj, x, values); grad x = the same kernel on the transposed pattern (values read through its
    permutation), grad values = sddmm_heads(grad_out, x)"""

    @staticmethod
    def forward(ctx, adj, x, values):
        xd, v = x.detach().contiguous(), values.detach().contiguous()
        heads = int(v.shape[1])
        out = _spmm_heads_raw(adj, adj.rowptr, adj.col, None, adj.m, v, xd, heads)
        ctx.adj, ctx.heads = adj, heads
        ctx.save_for_backward(xd, v)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        xd, v = ctx.saved_tensors
        adj = ctx.adj
        g = g.contiguous()
        gx = gv = None
        if ctx.needs_input_grad[1]:
            trp, trow, tperm = adj.tpattern()
            gx = _spmm_heads_raw(adj, trp, trow, tperm, adj.n, v, g, ctx.heads)
        if ctx.needs_input_grad[2]:
            gv = _sddmm_heads_raw(adj, g, xd, ctx.heads)
        return None, gx, gv


class _SddmmHeadsFunction(torch.autograd.Function):
    """s = sddmm_heads(adj, a, b); grad a = spmm_heads on the pattern (b weighted by grad s), grad b = spmm_heads on the
    transposed pattern (a weighted by grad s through the permutation)"""

    @staticmethod
    def forward(ctx, adj, a, b, heads):
        ad, bd = a.detach().contiguous(), b.detach().contiguous()
        ctx.adj, ctx.heads = adj, heads
        ctx.save_for_backward(ad, bd)
        return _sddmm_heads_raw(adj, ad, bd, heads)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        ad, bd = ctx.saved_tensors
        adj = ctx.adj
        g = g.contiguous()
        ga = gb = None
        if ctx.needs_input_grad[1]:
            ga = _spmm_heads_raw(adj, adj.rowptr, adj.col, None, adj.m, g, bd, ctx.heads)
        if ctx.needs_input_grad[2]:
            trp, trow, tperm = adj.tpattern()
            gb = _spmm_heads_raw(adj, trp, trow, tperm, adj.n, g, ad, ctx.heads)
        return None, ga, gb, None


def spmm_heads(adj, x, values):
    """out[r, hF + j] = sum over the stored entries e of row r of values[e, h] * x[col[e], hF + j]: the aggregation of all H
    heads in one walk of the adjacency (gcn_spmm_heads_csr_f32).  x: [n, H*F] fp32, head h in columns hF .. hF + F - 1;
    values: [nnz, H] fp32 in adj's CSR order (adj's own values are ignored; any CsrAdjacency, no plan is used).
    Differentiable in x (the same kernel on the transposed pattern) and in values (sddmm_heads)."""
    _check_adj(adj, "spmm_heads")
    if not isinstance(values, torch.Tensor) or values.dim() != 2 or values.shape[0] != adj.nnz or values.shape[1] < 1:
        raise ValueError(f"spmm_heads: values must be a 2-D tensor [nnz = {adj.nnz}, H] in CSR order")
    heads = int(values.shape[1])
    if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.shape[0] != adj.n or x.shape[1] < heads or x.shape[1] % heads:
        raise ValueError(f"spmm_heads: x must be a 2-D tensor [n = {adj.n}, H*F] with H = {heads} heads")
    _fp32_tensors([(x, (adj.n, None), "spmm_heads: x", f"a 2-D tensor [{adj.n}, {int(x.shape[1])}]"),
                   (values, (adj.nnz, None), "spmm_heads: values", f"a 2-D tensor [nnz = {adj.nnz}, H] in CSR order")])
    return _SpmmHeadsFunction.apply(adj, x, values)


def sddmm_heads(adj, a, b, heads):
    """s[e, h] = sum over j < F of a[row(e), hF + j] * b[col[e], hF + j] for every stored entry e of adj: per-head dot-product
    scores (gcn_sddmm_heads_csr_f32).  a: [m, H*F], b: [n, H*F] fp32; returns [nnz, H] in adj's CSR order.  Differentiable in
    a and b (spmm_heads on the pattern and on its transpose)."""
    _check_adj(adj, "sddmm_heads")
    heads = int(heads)
    if heads < 1:
        raise ValueError("sddmm_heads: heads must be at least 1")
    if not isinstance(a, torch.Tensor) or a.dim() != 2 or a.shape[1] < heads or a.shape[1] % heads:
        raise ValueError(f"sddmm_heads: a must be a 2-D tensor [m = {adj.m}, H*F] with H = {heads} heads")
    k = int(a.shape[1])
    _fp32_tensors([(a, (adj.m, k), "sddmm_heads: a", f"a 2-D tensor [{adj.m}, {k}]"),
                   (b, (adj.n, k), "sddmm_heads: b", f"a 2-D tensor [{adj.n}, {k}]")])
    return _SddmmHeadsFunction.apply(adj, a, b, heads)


# ---- GATv2 scores (gcn_amd/csrc/multihead.hip) -------------------------------------------------------------------------------------
def _gatv2_scratch(adj, device, heads, k):
    """the "gatv2" buffer of the adjacency, for the three GATv2 calls (gcn_gatv2_ws_bytes: a flag and the chunk partials of
    the backward's two sums): allocated at the first forward, so before a capture"""
    return adj._scratch.get("gatv2", _ws_need("gcn_gatv2_ws_bytes", int(adj.nnz), int(heads), int(k)), device)


def _gatv2_backward_raw(adj, rowptr, idx, perm, rows, own, other, att, slope, g, want_act):
    """(grad_own [rows, k], act_sums [rows, k] or None) of gcn_gatv2_scores_backward_csr_f32 over (rowptr, idx, perm)"""
    heads, k = int(att.shape[0]), int(own.shape[1])
    grad = torch.empty(rows, k, dtype=torch.float32, device=own.device)
    act = torch.empty(rows, k, dtype=torch.float32, device=own.device) if want_act else None
    if rows == 0 or adj.nnz == 0:
        return grad.zero_(), (act.zero_() if want_act else None)
    ws = _gatv2_scratch(adj, own.device, heads, k)
    call("gcn_gatv2_scores_backward_csr_f32", rowptr, idx, perm, rows, adj.nnz, heads, k, own, other, att, slope, g, grad, act,
         ws, ws.numel(), device=own.device)
    return grad, act


class _Gatv2ScoresFunction(torch.autograd.Function):
    """s = gatv2_scores(adj, h_dst, h_src, att); the backward recomputes t = h_dst[row] + h_src[col] in two row walks: the
    pattern gives grad h_dst and the [m, k] sums whose column sums are grad att, the transposed pattern gives grad h_src"""

    @staticmethod
    def forward(ctx, adj, h_dst, h_src, att, slope):
        hd, hs, a = h_dst.detach().contiguous(), h_src.detach().contiguous(), att.detach().contiguous()
        heads, k = int(a.shape[0]), int(hd.shape[1])
        out = torch.empty(adj.nnz, heads, dtype=torch.float32, device=hd.device)
        if adj.m and adj.nnz:
            ws = _gatv2_scratch(adj, hd.device, heads, k)
            call("gcn_gatv2_scores_csr_f32", adj.rowptr, adj.col, adj.m, adj.nnz, heads, k, hd, hs, a, slope, out, ws, ws.numel(),
                 device=hd.device)
        ctx.adj, ctx.slope = adj, slope
        ctx.save_for_backward(hd, hs, a)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        hd, hs, a = ctx.saved_tensors
        adj = ctx.adj
        g = g.contiguous()
        g_dst = g_src = g_att = None
        need_dst, need_src, need_att = ctx.needs_input_grad[1:4]
        if need_dst or need_att:
            g_dst, act = _gatv2_backward_raw(adj, adj.rowptr, adj.col, None, adj.m, hd, hs, a, ctx.slope, g, need_att)
            if need_att:
                g_att = act.sum(0).view_as(a)
            if not need_dst:
                g_dst = None
        if need_src:
            trp, trow, tperm = adj.tpattern()
            g_src, _ = _gatv2_backward_raw(adj, trp, trow, tperm, adj.n, hs, hd, a, ctx.slope, g, False)
        return None, g_dst, g_src, g_att, None


def gatv2_scores(adj, h_dst, h_src, att, negative_slope=0.2):
    """s[e, h] = sum over j < F of att[h, j] * leaky_relu(h_dst[row(e), hF + j] + h_src[col[e], hF + j], negative_slope) for
    every stored entry e of adj: the attention scores of GATv2 (Brody et al. 2022), computed per entry inside the kernel —
    no [nnz, H*F] array is formed, forward or backward (gcn_gatv2_scores_csr_f32).  h_dst: [m, H*F], h_src: [n, H*F],
    att: [H, F], all fp32; returns [nnz, H] in adj's CSR order, for edge_softmax and then spmm_heads.  Any CsrAdjacency,
    square or rectangular; its values are ignored.  Differentiable in all three operands (two row walks, on the pattern and
    on its transpose, and one [m, H*F] column sum); the same tensor may be passed as h_dst and h_src.  The derivative of
    leaky_relu at 0 is the slope."""
    _check_adj(adj, "gatv2_scores")
    if not isinstance(att, torch.Tensor) or att.dim() != 2 or att.shape[0] < 1 or att.shape[1] < 1:
        raise ValueError("gatv2_scores: att must be a 2-D tensor [H, F]")
    heads, k = int(att.shape[0]), int(att.shape[0]) * int(att.shape[1])
    _fp32_tensors([(h_dst, (adj.m, k), "gatv2_scores: h_dst", f"a 2-D tensor [{adj.m}, {k}]"),
                   (h_src, (adj.n, k), "gatv2_scores: h_src", f"a 2-D tensor [{adj.n}, {k}]"),
                   (att, (heads, None), "gatv2_scores: att", "a 2-D tensor [H, F]")])
    return _Gatv2ScoresFunction.apply(adj, h_dst, h_src, att, float(negative_slope))

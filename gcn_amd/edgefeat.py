"""Message passing with a feature vector per stored entry (DGL's ``u_add_e`` / ``u_mul_e`` followed by a reduce; the
aggregation of GINE, MPNN and CGConv):

    h = gcn_amd.edge_aggregate(adj, x, edge_feat, op="add", act="relu")          # h[r] = sum_e relu(x[col[e]] + edge_feat[e])
    h, arg = gcn_amd.edge_aggregate(adj, x, edge_feat, "mul", reduce="max", return_arg=True)

``edge_feat`` is [nnz, k] in the entry order of ``adj``; only the pattern of ``adj`` is used.  Everything runs on
gcn_amd/csrc/edge_message.hip: no [nnz, k] intermediate is formed or saved (the backward recomputes the message), no
atomics, the same bits at every call, and after one eager call of a width everything here runs inside a captured step.
There is no CPU path: CPU tensors raise.
"""
import torch

from . import _lib
from ._lib import call
from .aggregate import _scratch as _aggregate_scratch
from .spmm import CsrAdjacency

_CHUNK = 4096                # entries per workspace partial: GCN_EDGE_AGGREGATE_WS_BYTES in include/gcn_spmm.h
_OP = {"add": _lib.EDGE_OP_ADD, "mul": _lib.EDGE_OP_MUL}
_ACT = {None: _lib.EDGE_ACT_NONE, "relu": _lib.EDGE_ACT_RELU}
_REDUCE = {"sum": _lib.REDUCE_SUM, "mean": _lib.REDUCE_SUM, "max": _lib.REDUCE_MAX, "min": _lib.REDUCE_MIN}


def _ws_bytes(nnz, k):
    return 16 + 16 * int(k) * ((int(nnz) + _CHUNK - 1) // _CHUNK)


def _scratch(adj, k, device):
    """the "edge_aggregate" buffer of the adjacency (a flag and the partials of rows longer than 4096 entries), shared by
    the three kernels, which one stream orders; None for a pattern without entries (aggregate.py's rule)"""
    return adj._scratch.get("edge_aggregate", _ws_bytes(adj.nnz, k), device) if adj.nnz else None


def route(k, *tensors):
    """the form the kernels take for operands of width k at these addresses: (VEC, LPS, column tiles) — 16-byte accesses
    when every operand is 16-byte aligned and k % 4 == 0, then 16, 32 or 64 lanes a slot by k / VEC"""
    vec = 4 if k % 4 == 0 and all(t.data_ptr() % 16 == 0 for t in tensors) else 1
    units = k // vec
    lps = 16 if units <= 16 else 32 if units <= 32 else 64
    return vec, lps, (k + lps * vec - 1) // (lps * vec)


def _forward(adj, x, w, op, act, reduce, arg):
    k = int(x.shape[1])
    out = torch.empty((adj.m, k), dtype=torch.float32, device=x.device)
    ws = _scratch(adj, k, x.device)
    call("gcn_edge_aggregate_csr_f32", adj.rowptr, adj.col, adj.m, adj.n, adj.nnz, x, w, k, _OP[op], _ACT[act], _REDUCE[reduce],
         out, arg, ws, ws.numel() if ws is not None else 0, device=x.device)
    return out


class _SumFunction(torch.autograd.Function):
    """out[r] = sum over the entries e of row r of act(x[col[e]] op w[e]); both gradients from kernels that recompute it"""

    @staticmethod
    def forward(ctx, adj, x, w, op, act):
        x, w = x.detach().contiguous(), w.detach().contiguous()
        ctx.adj, ctx.op, ctx.act = adj, op, act
        ctx.save_for_backward(x, w)
        return _forward(adj, x, w, op, act, "sum", None)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        adj = ctx.adj
        g = g.contiguous()
        k = int(g.shape[1])
        ws = _scratch(adj, k, g.device)
        nws = ws.numel() if ws is not None else 0
        gx = ge = None
        if ctx.needs_input_grad[1]:
            gx = torch.empty((adj.n, k), dtype=torch.float32, device=g.device)
            trowptr, trow, tperm = adj.tpattern()
            call("gcn_edge_aggregate_backward_x_csr_f32", trowptr, trow, tperm, adj.n, adj.m, adj.nnz, g, x, w, k, _OP[ctx.op],
                 _ACT[ctx.act], gx, ws, nws, device=g.device)
        if ctx.needs_input_grad[2]:
            ge = torch.empty((adj.nnz, k), dtype=torch.float32, device=g.device)
            call("gcn_edge_aggregate_backward_e_csr_f32", adj.rowptr, adj.col, adj.m, adj.n, adj.nnz, g, x, w, k, _OP[ctx.op],
                 _ACT[ctx.act], ge, ws, nws, device=g.device)
        return None, gx, ge, None, None


class _SelectFunction(torch.autograd.Function):
    """(out, arg) = the row-wise max / min of the message and the entry that supplied it.  The gradient goes to that entry
    alone: element-wise [m, k] work on the recomputed winner, then the scatter-free backward of a selection for x and one
    non-accumulating index_put for edge_feat (its targets (arg[r, j], j) are distinct)."""

    @staticmethod
    def forward(ctx, adj, x, w, op, act, reduce):
        x, w = x.detach().contiguous(), w.detach().contiguous()
        arg = torch.empty((adj.m, int(x.shape[1])), dtype=torch.int32, device=x.device)
        out = _forward(adj, x, w, op, act, reduce, arg)
        ctx.adj, ctx.op, ctx.act = adj, op, act
        ctx.save_for_backward(x, w, arg)
        ctx.mark_non_differentiable(arg)
        return out, arg

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g, _g_arg):
        x, w, arg = ctx.saved_tensors
        adj, mul = ctx.adj, ctx.op == "mul"
        k = int(g.shape[1])
        gx = ge = None
        if adj.nnz == 0 or adj.m == 0:
            return (None, torch.zeros_like(x) if ctx.needs_input_grad[1] else None,
                    torch.zeros_like(w) if ctx.needs_input_grad[2] else None, None, None, None)
        live = arg >= 0
        ent = arg.clamp(min=0).long()                      # (an empty row reads entry 0 and contributes nothing)
        jj = torch.arange(k, device=g.device).expand_as(ent)
        x_arg = x[adj.col.long()[ent], jj]
        w_arg = w[ent, jj]
        if ctx.act == "relu":
            t = x_arg * w_arg if mul else x_arg + w_arg
            live = live & ~(t <= 0)                        # (threshold_backward: a NaN passes the gradient)
        gm = torch.where(live, g, torch.zeros((), dtype=g.dtype, device=g.device))
        if ctx.needs_input_grad[1]:
            gsel = (gm * w_arg if mul else gm).contiguous()
            gx = torch.empty((adj.n, k), dtype=torch.float32, device=g.device)
            trowptr, trow, tperm = adj.tpattern()
            ws = _aggregate_scratch(adj, k, g.device)
            call("gcn_aggregate_backward_csr", trowptr, trow, tperm, adj.n, adj.m, adj.nnz, gsel, _lib.DTYPE_F32, arg, k, gx,
                 ws, ws.numel() if ws is not None else 0, device=g.device)
        if ctx.needs_input_grad[2]:
            # one row more than w has: the entries of empty rows all land there (and nowhere that is kept)
            buf = torch.zeros((adj.nnz + 1, k), dtype=torch.float32, device=g.device)
            buf.index_put_((torch.where(arg >= 0, ent, torch.full_like(ent, adj.nnz)), jj), gm * x_arg if mul else gm)
            ge = buf[:adj.nnz]
        return None, gx, ge, None, None, None


def _row_counts(adj):
    """fp32 [m, 1]: the entry count of every row, 1 for an empty one (the mean's divisor), kept on the adjacency"""
    cnt = getattr(adj, "_edge_row_counts", None)
    if cnt is None:
        rp = adj.rowptr
        cnt = adj._edge_row_counts = (rp[1:] - rp[:-1]).clamp(min=1).to(torch.float32).unsqueeze(1)
    return cnt


def edge_aggregate(adj, x, edge_feat, op="add", act=None, reduce="sum", return_arg=False):
    """out[r, :] = the ``reduce`` over the stored entries e = (r, c) of row r of ``adj`` of act(x[c, :] op edge_feat[e, :]).

    adj: any CsrAdjacency; only its pattern is used and duplicates are separate entries.  x: [adj.n, k], edge_feat:
    [adj.nnz, k] in the entry order of ``adj`` (for a sampled block: ``edge_attr[block.eid.long()]``); both fp32 device
    tensors, differentiable (first derivatives).  op: "add" or "mul", one fp32 operation rounded once.  act: None or
    "relu" (NaN is kept; the derivative at 0 is 0).  reduce: "sum", "mean" (the sum divided once by the row's entry count),
    "max", "min" (ties go to the lowest entry index, -0.0 ties with +0.0, a NaN wins and the first NaN is reported; the
    gradient goes to the selected entry only).  An empty row gives zeros.  ``return_arg=True`` (max / min) also returns
    the int32 [m, k] entry indices that supplied the values, -1 for an empty row.
    TypeError for a non-CsrAdjacency, ValueError for a wrong shape or an unknown choice (or return_arg with sum / mean),
    GcnAmdError for a CPU tensor or a dtype other than fp32."""
    if not isinstance(adj, CsrAdjacency):
        raise TypeError("edge_aggregate: adj must be a CsrAdjacency")
    if op not in _OP:
        raise ValueError(f"edge_aggregate: op must be 'add' or 'mul', not {op!r}")
    if act not in _ACT:
        raise ValueError(f"edge_aggregate: act must be None or 'relu', not {act!r}")
    if reduce not in _REDUCE:
        raise ValueError(f"edge_aggregate: reduce must be 'sum', 'mean', 'max' or 'min', not {reduce!r}")
    if return_arg and reduce in ("sum", "mean"):
        raise ValueError("edge_aggregate: return_arg needs reduce='max' or 'min'")
    if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.shape[0] != adj.n or x.shape[1] < 1:
        raise ValueError(f"edge_aggregate: x must be a 2-D tensor of n = {adj.n} rows and at least one column")
    if not isinstance(edge_feat, torch.Tensor) or edge_feat.dim() != 2 or tuple(edge_feat.shape) != (adj.nnz, int(x.shape[1])):
        raise ValueError(f"edge_aggregate: edge_feat must be [nnz = {adj.nnz}, k = {int(x.shape[1])}]")
    if not (x.is_cuda and edge_feat.is_cuda):
        raise _lib.GcnAmdError("edge_aggregate: x and edge_feat must be CUDA/HIP tensors (no CPU path in gcn_amd)")
    if x.dtype != torch.float32 or edge_feat.dtype != torch.float32:
        raise _lib.GcnAmdError("edge_aggregate: x and edge_feat must be fp32")
    if reduce in ("max", "min"):
        out, arg = _SelectFunction.apply(adj, x, edge_feat, op, act, reduce)
        return (out, arg) if return_arg else out
    out = _SumFunction.apply(adj, x, edge_feat, op, act)
    return out / _row_counts(adj) if reduce == "mean" else out
